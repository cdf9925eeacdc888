// weights.hip -- model build: config defaults, weight sharding + re-layout into HBM, RoPE tables, activation scratch.
//
// Reference semantics reproduced here (all citations into /root/reference/src/models):
//   config defaults + validation   llama.rs:31-50, mistral.rs:93-154, qwen.rs:30-56, config.rs:31-54
//   weights bound by HF name       llama.rs:112-120, mistral.rs:190-192, qwen.rs:108-109
//
// HBM layout (per shard; compute dtype = bf16 or fp32):
//   wqkv [(Hs+2Hkvs)d, h]  fused q|k|v rows       wo [h, Hs*d]
//   wgu  [2*Ip, h] gate/up rows interleaved 16x16  wd [h, Ip]      (Ip = Is rounded up to 16)
//   lm_head [Vs, h], embed [V, h], norms fp32, RoPE cos/sin fp32 [max_pos][d/2]
#include "model.h"

#include <math.h>

#include <algorithm>
#include <memory>

namespace fl {

// ------------------------------------------------------------------------------- config
int resolve_config(const fl_config *cfg, Dims *o) {
    if (!cfg) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null config");
    Dims D;
    D.family = cfg->family;
    if (D.family < FL_FAMILY_LLAMA || D.family > FL_FAMILY_QWEN2) FL_FAIL(FL_ERR_BAD_CONFIG, "unknown model family %d", D.family);
    D.qkv_bias = cfg->qkv_bias != 0;
    D.h = cfg->hidden_size; D.inter = cfg->intermediate_size; D.V = cfg->vocab_size;
    D.L = cfg->num_hidden_layers; D.H = cfg->num_attention_heads;
    if (D.h <= 0 || D.inter <= 0 || D.V <= 0 || D.L <= 0 || D.H <= 0) FL_FAIL(FL_ERR_BAD_CONFIG, "non-positive model dimension");
    D.Hkv = cfg->num_key_value_heads > 0 ? cfg->num_key_value_heads : D.H;          // llama.rs:39
    D.dm = D.h / D.H;
    if (D.dm * D.H != D.h) FL_FAIL(FL_ERR_BAD_CONFIG, "hidden_size must be divisible by num_attention_heads");   // config.rs:34
    if (D.dm % 2) FL_FAIL(FL_ERR_BAD_CONFIG, "head_dim must be even for RoPE embeddings");                       // config.rs:39
    // The kernels are built for head_dim 64 and 128 (MFMA tiles, 16-byte rows).  Any other even head_dim up to 128 -- the reference
    // takes every even value (config.rs:31-43; e.g. 80, 96, 100) -- runs as the next of the two: every head's q / k / v rows are
    // laid out as [first half | zeros | second half | zeros] (so rotate-half pairs stay dm/2... d/2 apart) and o_proj gets zero
    // columns to match; the padded lanes carry exact zeros through RoPE, scores and values.  Above 128: fl_model_create refuses.
    D.d = D.dm <= 64 ? 64 : 128;
    if (D.H % D.Hkv) FL_FAIL(FL_ERR_BAD_CONFIG, "num_attention_heads must be divisible by num_key_value_heads"); // config.rs:48
    if (cfg->rms_norm_eps < 0) FL_FAIL(FL_ERR_BAD_CONFIG, "negative rms_norm_eps");
    D.eps = (float)cfg->rms_norm_eps;
    D.theta = cfg->rope_theta > 0 ? cfg->rope_theta : 10000.0;                                                   // llama.rs:41
    const int64_t dflt_pos = D.family == FL_FAMILY_LLAMA ? 4096 : 32768;                                        // llama.rs:47, mistral.rs:138
    D.max_pos = cfg->max_position_embeddings > 0 ? cfg->max_position_embeddings : dflt_pos;
    if (D.family == FL_FAMILY_LLAMA) D.window = -1;
    else D.window = cfg->sliding_window > 0 ? cfg->sliding_window : (cfg->sliding_window < 0 ? -1 : 4096);      // mistral.rs:139
    D.scale = (float)(1.0 / sqrt((double)D.dm));                                                                 // (the model's head_dim, not the padded one)
    *o = D;
    return FL_OK;
}

static bool ends_with(const std::string &s, const char *suf) {
    size_t n = strlen(suf); return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
}

// Megatron-style partition: q/k/v/gate/up/lm_head column-parallel (rows of the
// [out,in] matrix), o_proj/down_proj row-parallel (columns); norms and the embedding whole.
int tp_slice(const Dims &D, const char *name_c, int rank, int tp, int64_t out[4]) {
    if (tp < 1 || rank < 0 || rank >= tp) FL_FAIL(FL_ERR_BAD_ARGUMENT, "bad tp rank %d of %d", rank, tp);
    if (D.H % tp || D.Hkv % tp) FL_FAIL(FL_ERR_UNSUPPORTED, "tp=%d must divide heads (%lld) and kv heads (%lld)", tp, (long long)D.H, (long long)D.Hkv);
    if (D.inter % tp) FL_FAIL(FL_ERR_UNSUPPORTED, "tp=%d must divide intermediate_size %lld", tp, (long long)D.inter);
    const std::string name(name_c);
    const int64_t qd = D.H * D.dm, kvd = D.Hkv * D.dm;             // (source tensor coordinates: the model's head_dim)
    int64_t R = 0, C = 0, r0 = 0, r1 = 0, c0 = 0, c1 = 0;
    auto rows = [&](int64_t n, int64_t k) { R = n; C = k; r0 = n / tp * rank; r1 = n / tp * (rank + 1); c0 = 0; c1 = k; };
    auto cols = [&](int64_t n, int64_t k) { R = n; C = k; r0 = 0; r1 = n; c0 = k / tp * rank; c1 = k / tp * (rank + 1); };
    auto whole = [&](int64_t n, int64_t k) { R = n; C = k; r0 = 0; r1 = n; c0 = 0; c1 = k; };
    if (ends_with(name, "q_proj.weight")) rows(qd, D.h);
    else if (ends_with(name, "k_proj.weight") || ends_with(name, "v_proj.weight")) rows(kvd, D.h);
    else if (ends_with(name, "q_proj.bias")) rows(qd, 1);
    else if (ends_with(name, "k_proj.bias") || ends_with(name, "v_proj.bias")) rows(kvd, 1);
    else if (ends_with(name, "o_proj.weight")) cols(D.h, qd);
    else if (ends_with(name, "gate_proj.weight") || ends_with(name, "up_proj.weight")) rows(D.inter, D.h);
    else if (ends_with(name, "down_proj.weight")) cols(D.h, D.inter);
    else if (name == "lm_head.weight") { if (D.V % tp == 0) rows(D.V, D.h); else whole(D.V, D.h); }
    else if (name == "model.embed_tokens.weight") whole(D.V, D.h);
    else if (ends_with(name, "layernorm.weight") || name == "model.norm.weight") whole(D.h, 1);
    else FL_FAIL(FL_ERR_MISSING_TENSOR, "unknown tensor name %s", name_c);
    (void)R; (void)C;
    out[0] = r0; out[1] = r1; out[2] = c0; out[3] = c1;
    return FL_OK;
}

// ------------------------------------------------------------------------------- allocation
static std::atomic<int> g_poison_count{0};
void tune_poison_restart() { g_poison_count.store(0); }
int dev_alloc(std::vector<void *> &owner, void **p, size_t bytes, int64_t *acct) {
    if (bytes == 0) bytes = 16;
    const hipError_t e = hipMalloc(p, bytes);
    if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); FL_FAIL(FL_ERR_OOM, "out of HBM: hipMalloc of %zu bytes failed", bytes); }
    FL_HIP(e);
    owner.push_back(*p);
    if (acct) *acct += (int64_t)bytes;
    if (const int fill = tune(TK_DEBUG_POISON)) {
        // bits 0-7: the byte; bits 8+: 0 = every allocation, n = only the n-th since the switch was last set (tools/poison_probe.py scans)
        const int nth = g_poison_count.fetch_add(1) + 1, want = fill >> 8;
        if (want == 0 || want == nth) { FL_HIP(hipMemset(*p, fill & 0xFF, bytes)); FL_HIP(hipDeviceSynchronize()); }
    }
    return FL_OK;
}

Model::~Model() {
    std::vector<hipStream_t> closed;            // EMULATED shards share one stream
    for (auto &s : shards) {
        (void)hipSetDevice(s.device);
        if (s.stream) (void)hipStreamSynchronize(s.stream);
        if (s.comm) ncclCommDestroy(s.comm);
        if (s.comm_stream) { (void)hipStreamSynchronize(s.comm_stream); (void)hipStreamDestroy(s.comm_stream); }
        for (auto &e : s.ev) if (e) (void)hipEventDestroy(e);
        for (void *mp : s.pc.mapped) if (mp) (void)hipIpcCloseMemHandle(mp);
        if (s.pc.local) { comm_forget(s.pc.local); comm_inbox_release(s.device, s.pc.bytes, s.pc.local); }
        if (s.pc.epoch) (void)hipFree(s.pc.epoch);
        if (s.pc.ll_dev) (void)hipFree(s.pc.ll_dev);
        if (s.pc.err) (void)hipHostFree(s.pc.err);
        for (void *p : s.allocs) (void)hipFree(p);
        for (void *p : s.pre_allocs) (void)hipFree(p);
        for (void *p : s.packed.allocs) (void)hipFree(p);
        if (s.packed.tab) (void)hipFree(s.packed.tab);
        if (s.packed.host_tab) (void)hipHostFree(s.packed.host_tab);
        if (s.packed.host_result) (void)hipHostFree(s.packed.host_result);
        if (s.packed.host_verify) (void)hipHostFree(s.packed.host_verify);
        if (s.packed.verify_prob) (void)hipFree(s.packed.verify_prob);
        if (s.packed.embed_out) (void)hipFree(s.packed.embed_out);
        if (s.packed.embed_part) (void)hipFree(s.packed.embed_part);
        if (s.score.rows) (void)hipFree(s.score.rows);
        if (s.score.targets) (void)hipFree(s.score.targets);
        if (s.score.recs) (void)hipFree(s.score.recs);
        if (s.score.host_targets) (void)hipHostFree(s.score.host_targets);
        if (s.score.host_recs) (void)hipHostFree(s.score.host_recs);
        if (s.stream && std::find(closed.begin(), closed.end(), s.stream) == closed.end()) {
            closed.push_back(s.stream);
            gemm_8p_release_stream(s.stream);
            gemm_h4_release_stream(s.stream);
            gemm_skf_release_stream(s.stream);
            (void)hipStreamDestroy(s.stream);
        }
    }
    if (emu_ptrs) (void)hipFree(emu_ptrs);
    if (host_logits) (void)hipHostFree(host_logits);
    if (host_tokens) (void)hipHostFree(host_tokens);
    if (host_verify) (void)hipHostFree(host_verify);
    if (host_verify_recs) (void)hipHostFree(host_verify_recs);
    if (host_state) (void)hipHostFree(host_state);
    if (host_lp) (void)hipHostFree(host_lp);
    for (auto &r : prof) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
}

// ------------------------------------------------------------------------------- weight build
struct Stager {                      // brings a source tensor to a device (whole), reusing one buffer
    int device; void *buf = nullptr; size_t cap = 0;
    explicit Stager(int dev) : device(dev) {}
    ~Stager() { if (buf) { (void)hipSetDevice(device); (void)hipFree(buf); } }
    int get(const fl_tensor &t, size_t bytes, const void **out) {
        if (t.device == device) { *out = t.data; return FL_OK; }
        if (bytes > cap) {
            if (buf) { FL_HIP(hipFree(buf)); buf = nullptr; cap = 0; }
            FL_HIP(hipMalloc(&buf, bytes)); cap = bytes;
        }
        FL_HIP(hipMemcpy(buf, t.data, bytes, hipMemcpyDefault));
        *out = buf;
        return FL_OK;
    }
};

static size_t dtype_size(int dt) { return dt == FL_DTYPE_F32 ? 4 : 2; }

struct Builder {
    Model *m;
    std::unordered_map<std::string, const fl_tensor *> map;
    const fl_tensor *find(const std::string &name) const {
        auto it = map.find(name); return it == map.end() ? nullptr : it->second;
    }
    int want(const std::string &name, int64_t R, int64_t C, const fl_tensor **out) const {
        const fl_tensor *t = find(name);
        if (!t) FL_FAIL(FL_ERR_MISSING_TENSOR, "cannot find tensor %s", name.c_str());
        if (t->dtype < FL_DTYPE_F32 || t->dtype > FL_DTYPE_F16) FL_FAIL(FL_ERR_UNSUPPORTED, "tensor %s: unsupported dtype %d", name.c_str(), t->dtype);
        bool ok = (C == 1 && t->ndim == 1) ? t->shape[0] == R : (t->ndim == 2 && t->shape[0] == R && t->shape[1] == C);
        if (!ok) FL_FAIL(FL_ERR_SHAPE_MISMATCH, "shape mismatch for %s: expected [%lld,%lld]", name.c_str(), (long long)R, (long long)C);
        if (!t->data) FL_FAIL(FL_ERR_BAD_ARGUMENT, "tensor %s has null data", name.c_str());
        *out = t; return FL_OK;
    }
};

// Copy slice [r0,r1) x [c0,c1) of tensor `name` (full shape R x C) into dst (ld = dst_ld) on every
// shard that lives on st.device; dst_of(shard) gives the destination base, row_mode the row map.
// head_pad: 0 none; 1 the ROWS are heads of the model's head_dim dm, placed as padded heads of d rows; 2 the COLUMNS are
// An fp32 destination of a bf16 model (norm weights, q/k/v biases) takes the value ROUNDED TO BF16: the reference casts every tensor
// of the checkpoint to the model's dtype (VarBuilder::from_tensors(tensors, dtype, device), llama.rs:112, mistral.rs:190, qwen.rs:108),
// so an f32 or f16 checkpoint served in bf16 has bf16 norm weights and biases; the fp32 copy only spares the kernels a conversion.
template <typename DstFn>
static int put_matrix(Builder &B, Stager &st, const std::string &name, int64_t R, int64_t C, int dst_dtype,
                      int64_t dst_ld, int64_t dst_row0, int row_mode, DstFn dst_of, int head_pad = 0) {
    Model *m = B.m;
    const fl_tensor *t = nullptr;
    FL_TRY(B.want(name, R, C, &t));
    const void *src = nullptr;
    FL_TRY(st.get(*t, (size_t)R * C * dtype_size(t->dtype), &src));
    for (auto &sh : m->shards) {
        if (sh.device != st.device) continue;
        int64_t sl[4];
        FL_TRY(tp_slice(m->D, name.c_str(), sh.rank, m->tp, sl));
        Launcher L; L.stream = sh.stream;
        FL_TRY(launch_convert_slice(L, t->dtype, src, C, sl[0], sl[2], sl[1] - sl[0], sl[3] - sl[2], dst_dtype,
                                    dst_of(sh), dst_ld, dst_row0, row_mode, m->D.dm != m->D.d ? head_pad : 0, m->D.dm, m->D.d,
                                    dst_dtype == FL_DTYPE_F32 && m->dtype == FL_DTYPE_BF16));
    }
    FL_HIP(hipDeviceSynchronize());       // the staging buffer is reused by the next tensor
    return FL_OK;
}

static int build_weights(Builder &B) {
    Model *m = B.m;
    const Dims &D = m->D;
    const int wdt = m->dtype;
    const size_t es = m->esize();
    std::vector<int> devices;
    for (auto &sh : m->shards) if (std::find(devices.begin(), devices.end(), sh.device) == devices.end()) devices.push_back(sh.device);

    // allocate: one arena per shard (FL_WEIGHT_ARENA=0: one hipMalloc per tensor).  The whole model is then a single
    // virtual range, which the driver can map with its largest page fragments
    const int use_arena = tune(TK_WEIGHT_ARENA);
    for (auto &sh : m->shards) {
        FL_HIP(hipSetDevice(sh.device));
        const int64_t nq = (sh.Hs + 2 * sh.Hkvs) * D.d;
        char *arena = nullptr; size_t arena_off = 0, arena_cap = 0;
        auto walloc = [&](void **p, size_t bytes) -> int {
            if (!arena) return dev_alloc(sh.allocs, p, bytes, &m->hbm_bytes);
            const size_t a = (bytes + 4095) & ~(size_t)4095;
            if (arena_off + a > arena_cap) FL_FAIL(FL_ERR_OOM, "weight arena too small");
            *p = arena + arena_off; arena_off += a;
            return FL_OK;
        };
        if (use_arena) {
            auto r4k = [](size_t b) { return (b + 4095) & ~(size_t)4095; };
            size_t need = r4k((size_t)D.V * D.h * es) + r4k((size_t)D.h * 4) + r4k((size_t)sh.Vs * D.h * es);
            need += (size_t)D.L * (r4k((size_t)nq * D.h * es) + r4k((size_t)nq * 4) + r4k((size_t)D.h * sh.Hs * D.d * es) +
                                   r4k((size_t)2 * sh.Ip * D.h * es) + r4k((size_t)D.h * sh.Ip * es) + 2 * r4k((size_t)D.h * 4));
            FL_TRY(dev_alloc(sh.allocs, (void **)&arena, need, &m->hbm_bytes));
            arena_cap = need;
        }
        FL_TRY(walloc(&sh.embed, (size_t)D.V * D.h * es));
        FL_TRY(walloc((void **)&sh.norm, (size_t)D.h * 4));
        FL_TRY(walloc(&sh.lm_head, (size_t)sh.Vs * D.h * es));
        sh.layers.resize(D.L);
        for (auto &ly : sh.layers) {
            FL_TRY(walloc(&ly.wqkv, (size_t)nq * D.h * es));
            if (D.qkv_bias) FL_TRY(walloc((void **)&ly.bqkv, (size_t)nq * 4));
            FL_TRY(walloc(&ly.wo, (size_t)D.h * sh.Hs * D.d * es));
            FL_TRY(walloc(&ly.wgu, (size_t)2 * sh.Ip * D.h * es));
            FL_TRY(walloc(&ly.wd, (size_t)D.h * sh.Ip * es));
            FL_TRY(walloc((void **)&ly.ln1, (size_t)D.h * 4));
            FL_TRY(walloc((void **)&ly.ln2, (size_t)D.h * 4));
            if (D.dm != D.d) {               // padded head_dim: the rows / columns between the halves of every head stay zero
                FL_HIP(hipMemsetAsync(ly.wqkv, 0, (size_t)nq * D.h * es, sh.stream));
                if (D.qkv_bias) FL_HIP(hipMemsetAsync(ly.bqkv, 0, (size_t)nq * 4, sh.stream));
                FL_HIP(hipMemsetAsync(ly.wo, 0, (size_t)D.h * sh.Hs * D.d * es, sh.stream));
            }
            if (sh.Ip != sh.Is) {            // zero padding rows/cols so they contribute nothing
                FL_HIP(hipMemsetAsync(ly.wgu, 0, (size_t)2 * sh.Ip * D.h * es, sh.stream));
                FL_HIP(hipMemsetAsync(ly.wd, 0, (size_t)D.h * sh.Ip * es, sh.stream));
            }
        }
        FL_HIP(hipStreamSynchronize(sh.stream));
    }

    const bool has_lm_head = B.find("lm_head.weight") != nullptr;
    if (!has_lm_head && D.family != FL_FAMILY_QWEN2) FL_FAIL(FL_ERR_MISSING_TENSOR, "cannot find tensor lm_head.weight");

    for (int dev : devices) {
        FL_HIP(hipSetDevice(dev));
        Stager st(dev);
        FL_TRY(put_matrix(B, st, "model.embed_tokens.weight", D.V, D.h, wdt, D.h, 0, 0, [](Shard &s) { return s.embed; }));
        FL_TRY(put_matrix(B, st, "model.norm.weight", D.h, 1, FL_DTYPE_F32, 1, 0, 0, [](Shard &s) { return (void *)s.norm; }));
        if (has_lm_head) {
            FL_TRY(put_matrix(B, st, "lm_head.weight", D.V, D.h, wdt, D.h, 0, 0, [](Shard &s) { return s.lm_head; }));
        } else {
            // candle qwen2 falls back to the embedding matrix when lm_head.weight is absent (App. A.1)
            const fl_tensor *t = nullptr; const void *src = nullptr;
            FL_TRY(B.want("model.embed_tokens.weight", D.V, D.h, &t));
            FL_TRY(st.get(*t, (size_t)D.V * D.h * dtype_size(t->dtype), &src));
            for (auto &sh : m->shards) {
                if (sh.device != dev) continue;
                Launcher L; L.stream = sh.stream;
                FL_TRY(launch_convert_slice(L, t->dtype, src, D.h, sh.v0, 0, sh.Vs, D.h, wdt, sh.lm_head, D.h, 0, 0));
            }
            FL_HIP(hipDeviceSynchronize());
        }
        for (int64_t l = 0; l < D.L; l++) {
            const std::string p = "model.layers." + std::to_string(l) + ".";
            auto LY = [l](Shard &s) -> LayerW & { return s.layers[l]; };
            const int64_t qd = D.H * D.dm, kvd = D.Hkv * D.dm;       // (source tensors: the model's head_dim)
            // fused q|k|v: destination row offsets inside the shard's fused matrix
            struct { const char *nm; int64_t R; int which; } qkv[3] = {{"self_attn.q_proj", qd, 0}, {"self_attn.k_proj", kvd, 1}, {"self_attn.v_proj", kvd, 2}};
            for (auto &e : qkv) {
                // all local shards have equal Hs / Hkvs, so the row offset is shard-independent
                const Shard &s0 = m->shards[0];
                const int64_t off = e.which == 0 ? 0 : (e.which == 1 ? s0.Hs * D.d : (s0.Hs + s0.Hkvs) * D.d);
                FL_TRY(put_matrix(B, st, p + e.nm + ".weight", e.R, D.h, wdt, D.h, off, 0, [&](Shard &s) { return LY(s).wqkv; }, 1));
                if (D.qkv_bias)
                    FL_TRY(put_matrix(B, st, p + e.nm + ".bias", e.R, 1, FL_DTYPE_F32, 1, off, 0, [&](Shard &s) { return (void *)LY(s).bqkv; }, 1));
            }
            FL_TRY(put_matrix(B, st, p + "self_attn.o_proj.weight", D.h, qd, wdt, m->shards[0].Hs * D.d, 0, 0, [&](Shard &s) { return LY(s).wo; }, 2));
            FL_TRY(put_matrix(B, st, p + "mlp.gate_proj.weight", D.inter, D.h, wdt, D.h, 0, 1, [&](Shard &s) { return LY(s).wgu; }));
            FL_TRY(put_matrix(B, st, p + "mlp.up_proj.weight", D.inter, D.h, wdt, D.h, 0, 2, [&](Shard &s) { return LY(s).wgu; }));
            FL_TRY(put_matrix(B, st, p + "mlp.down_proj.weight", D.h, D.inter, wdt, m->shards[0].Ip, 0, 0, [&](Shard &s) { return LY(s).wd; }));
            FL_TRY(put_matrix(B, st, p + "input_layernorm.weight", D.h, 1, FL_DTYPE_F32, 1, 0, 0, [&](Shard &s) { return (void *)LY(s).ln1; }));
            FL_TRY(put_matrix(B, st, p + "post_attention_layernorm.weight", D.h, 1, FL_DTYPE_F32, 1, 0, 0, [&](Shard &s) { return (void *)LY(s).ln2; }));
        }
    }
    return FL_OK;
}

// FL_WEIGHTS_E4M3_ROW: every projection matrix (in its final decode layout: a row scale follows its row through every row
// permutation) gets its e4m3 bytes and row scales, and the bf16 matrix itself becomes the image s * q -- what prefill, batches
// and every other bf16 kernel then read.  Both images stay: 1.5x a bf16 model's weight memory.
static int quantize_weights(Model *m) {
    const Dims &D = m->D;
    for (auto &sh : m->shards) {
        FL_HIP(hipSetDevice(sh.device));
        Launcher L; L.stream = sh.stream;
        auto one = [&](void *w, int64_t N, int64_t K, uint8_t **q, float **s) -> int {
            if (!gemv_w8_supported(N, K)) FL_FAIL(FL_ERR_UNSUPPORTED, "FL_WEIGHTS_E4M3_ROW: a %lld x %lld projection (K must be a multiple of 16)", (long long)N, (long long)K);
            FL_TRY(dev_alloc(sh.allocs, (void **)q, (size_t)N * K, &m->hbm_bytes));
            FL_TRY(dev_alloc(sh.allocs, (void **)s, (size_t)N * 4, &m->hbm_bytes));
            return launch_quantize_rows(L, FL_DTYPE_BF16, w, N, K, *q, *s, w);
        };
        const int64_t nq = (sh.Hs + 2 * sh.Hkvs) * D.d;
        for (auto &ly : sh.layers) {
            FL_TRY(one(ly.wqkv, nq, D.h, &ly.wqkv8, &ly.sqkv));
            FL_TRY(one(ly.wo, D.h, sh.Hs * D.d, &ly.wo8, &ly.so));
            FL_TRY(one(ly.wgu, 2 * sh.Ip, D.h, &ly.wgu8, &ly.sgu));
            FL_TRY(one(ly.wd, D.h, sh.Ip, &ly.wd8, &ly.sd));
        }
        FL_TRY(one(sh.lm_head, sh.Vs, D.h, &sh.lm_head8, &sh.lm_head_s));
        FL_HIP(hipStreamSynchronize(sh.stream));
    }
    return FL_OK;
}

// RoPE tables (App. A.4): inv_freq[j] = 1 / theta^(2j/d) in fp32; angle = p * inv_freq[j] (fp32
// product); cos/sin in fp32.  Built once on the host, one copy per shard.
static int build_rope(Model *m) {
    const Dims &D = m->D;
    const int64_t half = D.d / 2, half_m = D.dm / 2;             // pairs of the padded layout; of them, the model's (the rest rotate zeros: identity)
    std::vector<float> inv(half), c((size_t)D.max_pos * half), s((size_t)D.max_pos * half);
    const float theta = (float)D.theta;
    for (int64_t j = 0; j < half_m; j++) inv[j] = 1.0f / powf(theta, (float)(2 * j) / (float)D.dm);
    for (int64_t p = 0; p < D.max_pos; p++)
        for (int64_t j = 0; j < half; j++) {
            const float ang = j < half_m ? (float)p * inv[j] : 0.0f;
            c[(size_t)p * half + j] = cosf(ang);
            s[(size_t)p * half + j] = sinf(ang);
        }
    for (auto &sh : m->shards) {
        FL_HIP(hipSetDevice(sh.device));
        FL_TRY(dev_alloc(sh.allocs, (void **)&sh.cos_tab, c.size() * 4, &m->hbm_bytes));
        FL_TRY(dev_alloc(sh.allocs, (void **)&sh.sin_tab, s.size() * 4, &m->hbm_bytes));
        FL_HIP(hipMemcpy(sh.cos_tab, c.data(), c.size() * 4, hipMemcpyHostToDevice));
        FL_HIP(hipMemcpy(sh.sin_tab, s.data(), s.size() * 4, hipMemcpyHostToDevice));
    }
    return FL_OK;
}

// K slices (fp32 slabs that the next launch -- rmsnorm_add, rope_kv -- sums) a projection may use at T tokens.  Mid-size
// prompts (T = 256..1024: 1-4 row tiles of 256) get up to eight: on the 256x256 kernel Mistral-7B's T = 512 QKV takes
// 47 -> 34.5 us at 5 slices of 12.8 K steps, down_proj 78 -> 59 us at 8 (tools/gemm_probe.py), for ~5 us more in each summing launch.
static int mid_cap(int dflt) { const int v = tune(TK_KSPLIT_MID); return v > 0 ? std::min(v, kMaxKSplitMid) : dflt; }   // (read per call: A/B tools lower it on a live model; the slabs were sized for the default)
int ksplit_cap(int64_t T) { return T <= 1 ? 1 : (T > 128 && T <= kMidT ? mid_cap(kMaxKSplitMid) : kMaxKSplit); }
static int qkv_split_cap(int64_t T) { return T <= 1 ? 1 : (T <= 128 ? kMaxQkvSplitShort : (T <= kMidT ? mid_cap(kMaxKSplitMid) : kMaxQkvSplit)); }
// the same caps with the switch at its largest value: what the slab buffers are SIZED for (a later, larger FL_KSPLIT_MID must
// never write past a buffer that was allocated while it was lowered)
static int ksplit_cap_max(int64_t T) { return T <= 1 ? 1 : (T > 128 && T <= kMidT ? kMaxKSplitMid : kMaxKSplit); }
static int qkv_split_cap_max(int64_t T) { return T <= 1 ? 1 : (T <= 128 ? kMaxQkvSplitShort : (T <= kMidT ? kMaxKSplitMid : kMaxQkvSplit)); }
int qkv_split(int64_t T) { return std::min(tune(TK_QKV_SPLIT), qkv_split_cap(T)); }   // K slabs a prompt's QKV projection may leave
// rows of slab storage that serve every prompt of at most T tokens
static int64_t slab_rows(int64_t T, int (*cap)(int64_t)) {
    return std::max<int64_t>({T * cap(T), std::min<int64_t>(T, kMidT) * cap(std::min<int64_t>(T, kMidT)), std::min<int64_t>(T, 128) * cap(std::min<int64_t>(T, 128))});
}

int alloc_scratch(Model *m, Shard &sh, Scratch &sc, int64_t T, std::vector<void *> *owner) {
    std::vector<void *> &own = owner ? *owner : sh.allocs;
    int64_t *acct = (owner && owner != &sh.pre_allocs) ? nullptr : &m->hbm_bytes;
    const Dims &D = m->D;
    const size_t es = m->esize();
    const int64_t nq = (sh.Hs + 2 * sh.Hkvs) * D.d;
    sc.cap_T = T;
    FL_TRY(dev_alloc(own, (void **)&sc.x_res, (size_t)T * D.h * 4, acct));
    if (T == 1) FL_TRY(dev_alloc(own, (void **)&sc.x_res2, (size_t)D.h * 4, acct));
    if (T == 1 && m->dtype == FL_DTYPE_BF16) {
        FL_TRY(dev_alloc(own, &sc.xs_res, (size_t)D.h * 2, acct));
        FL_TRY(dev_alloc(own, (void **)&sc.cs_res, (size_t)(D.h + 7) / 8 * 4, acct));
    }
    // split-K slabs of any prompt <= T; decode: one partial vector per kv head (fused attention + o_proj launch)
    FL_TRY(dev_alloc(own, (void **)&sc.delta, (size_t)std::max<int64_t>(slab_rows(T, ksplit_cap_max), T == 1 ? sh.Hkvs : 0) * D.h * 4, acct));
    FL_TRY(dev_alloc(own, &sc.xn, (size_t)T * D.h * es, acct));
    FL_TRY(dev_alloc(own, (void **)&sc.inv_rms, (size_t)T * 4, acct));
    if (T > 1) FL_TRY(dev_alloc(own, (void **)&sc.rs_part, (size_t)T * gemm_resid_partials(D.h) * 4, acct));
    FL_TRY(dev_alloc(own, (void **)&sc.qkv, (size_t)slab_rows(T, qkv_split_cap_max) * nq * 4, acct));    // split-K slabs of any prompt <= T
    FL_TRY(dev_alloc(own, &sc.q, (size_t)T * sh.Hs * D.d * es, acct));
    FL_TRY(dev_alloc(own, &sc.ao, (size_t)T * sh.Hs * D.d * es, acct));
    FL_TRY(dev_alloc(own, &sc.act, (size_t)T * sh.Ip * es, acct));
    FL_TRY(dev_alloc(own, (void **)&sc.ids, (size_t)T * 4, acct));
    return FL_OK;
}

// The prefill scratch of a shard grows geometrically and the set it replaces is freed: every forward() ends with a
// stream synchronisation, so under the model mutex the old buffers are idle (a long-running server that sees longer
// and longer prompts would otherwise pile up one dead set per new maximum, ~180 KB per token for Mistral-7B).
int grow_prefill_scratch(Model *m, Shard &sh, int64_t T) {
    const int64_t chunk_max = tune(TK_PREFILL_CHUNK);
    int64_t cap = std::max<int64_t>(T, std::min<int64_t>(chunk_max, sh.pre.cap_T + sh.pre.cap_T / 2));
    cap = std::min<int64_t>(std::max<int64_t>(T, chunk_max), (cap + 127) / 128 * 128);
    FL_HIP(hipStreamSynchronize(sh.stream));
    if (sh.comm_stream) FL_HIP(hipStreamSynchronize(sh.comm_stream));
    for (void *p : sh.pre_allocs) (void)hipFree(p);
    sh.pre_allocs.clear();
    m->hbm_bytes -= sh.pre_bytes;
    sh.pre = Scratch{};
    const int64_t before = m->hbm_bytes;
    int rc = alloc_scratch(m, sh, sh.pre, cap, &sh.pre_allocs);
    if (rc != FL_OK) {                                   // leave the shard without a prefill scratch rather than with half of one
        for (void *p : sh.pre_allocs) (void)hipFree(p);
        sh.pre_allocs.clear(); sh.pre = Scratch{}; sh.pre_bytes = 0; m->hbm_bytes = before;
        return rc;
    }
    sh.pre_bytes = m->hbm_bytes - before;
    return FL_OK;
}

int model_create(const fl_config *cfg, const fl_tensor *tensors, size_t n, int compute_dtype,
                 const fl_parallel *par, const fl_model_options *opts, Model **out) {
    if (!out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null out pointer");
    if (!tensors && n) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null tensors");
    if (compute_dtype != FL_DTYPE_BF16 && compute_dtype != FL_DTYPE_F32)
        FL_FAIL(FL_ERR_UNSUPPORTED, "compute dtype must be BF16 (reference default, main.rs:120) or F32");
    Dims D;
    FL_TRY(resolve_config(cfg, &D));
    if (D.h % 8) FL_FAIL(FL_ERR_UNSUPPORTED, "hidden_size must be a multiple of 8 (16-byte rows)");
    if (D.dm > 128) FL_FAIL(FL_ERR_UNSUPPORTED, "head_dim %lld not supported (even values up to 128)", (long long)D.dm);
    if (D.max_pos > (1 << 20)) D.max_pos = 1 << 20;
    // options (fl_model_create_opts): everything that needs no device is decided here, before the device probe
    int decode_weights = FL_WEIGHTS_COMPUTE_DTYPE;
    if (opts) {
        if (opts->struct_size != sizeof(fl_model_options))
            FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_model_options.struct_size is %u, this library's is %zu", opts->struct_size, sizeof(fl_model_options));
        decode_weights = opts->decode_weights;
        if (decode_weights != FL_WEIGHTS_COMPUTE_DTYPE && decode_weights != FL_WEIGHTS_E4M3_ROW)
            FL_FAIL(FL_ERR_BAD_ARGUMENT, "unknown decode_weights %d (fl_weight_format)", decode_weights);
    }
    if (decode_weights == FL_WEIGHTS_E4M3_ROW) {
        if (compute_dtype != FL_DTYPE_BF16) FL_FAIL(FL_ERR_UNSUPPORTED, "FL_WEIGHTS_E4M3_ROW needs compute dtype BF16 (s * q is exact in bf16, the fp32 mode has no use for it)");
        if (par && par->mode != FL_TP_NONE && par->tp_size > 1) FL_FAIL(FL_ERR_UNSUPPORTED, "FL_WEIGHTS_E4M3_ROW does not support tensor parallelism (tp_size %d)", par->tp_size);
        // a lane of the FP8 stream loads 16 weights: every projection's K (hidden_size, heads x padded head_dim, intermediate_size
        // padded to 16) is a multiple of 16 once hidden_size is
        if (D.h % 16) FL_FAIL(FL_ERR_UNSUPPORTED, "FL_WEIGHTS_E4M3_ROW needs hidden_size to be a multiple of 16 (it is %lld)", (long long)D.h);
    }
    debug_inject("model_create");

    int ndev = 0;
    FL_TRY(require_device(&ndev));

    fl_parallel P{};
    if (par) P = *par;
    if (P.mode == FL_TP_NONE) { P.tp_size = 1; P.tp_rank = 0; }
    if (P.tp_size < 1) FL_FAIL(FL_ERR_BAD_ARGUMENT, "tp_size must be >= 1");
    const int tp = P.tp_size;
    if (D.H % tp || D.Hkv % tp || D.inter % tp)
        FL_FAIL(FL_ERR_UNSUPPORTED, "tp=%d must divide heads %lld, kv heads %lld and intermediate %lld", tp,
                (long long)D.H, (long long)D.Hkv, (long long)D.inter);

    std::unique_ptr<Model> m(new Model());
    m->D = D; m->dtype = compute_dtype; m->tp = tp; m->tp_mode = P.mode;
    m->vocab_parallel = tp > 1 && D.V % tp == 0;
    m->cfg_resolved = *cfg;
    m->cfg_resolved.num_key_value_heads = D.Hkv; m->cfg_resolved.rope_theta = D.theta;
    m->cfg_resolved.max_position_embeddings = D.max_pos; m->cfg_resolved.sliding_window = D.window;
    m->use_graph = tune(TK_GRAPH) != 0;                 // (-1 = automatic: on)
    m->fused_decode = tune(TK_FUSED) != 0 && gemv_norm_supported(compute_dtype, 1, D.h);
    m->decode_weights = decode_weights;
    if (decode_weights == FL_WEIGHTS_E4M3_ROW && (!m->fused_decode || !gemv_w8_norm_supported(1, D.h)))
        FL_FAIL(FL_ERR_UNSUPPORTED, "FL_WEIGHTS_E4M3_ROW needs the fused decode step (FL_FUSED=0, or hidden_size %lld above 6144)", (long long)D.h);

    auto dev_of = [&](int i) -> int { return (P.device_ids && i < P.n_device_ids) ? P.device_ids[i] : i; };
    int nlocal = 1;
    if (P.mode == FL_TP_SINGLE_PROCESS || P.mode == FL_TP_EMULATED) nlocal = tp;
    m->shards.resize(nlocal);
    for (int i = 0; i < nlocal; i++) {
        Shard &sh = m->shards[i];
        switch (P.mode) {
            case FL_TP_NONE: sh.rank = 0; sh.device = P.device_ids && P.n_device_ids > 0 ? P.device_ids[0] : 0; break;
            case FL_TP_SINGLE_PROCESS: sh.rank = i; sh.device = dev_of(i); break;
            case FL_TP_MULTI_PROCESS: sh.rank = P.tp_rank; sh.device = P.device_ids && P.n_device_ids > 0 ? P.device_ids[0] : 0; break;
            case FL_TP_EMULATED: sh.rank = i; sh.device = P.device_ids && P.n_device_ids > 0 ? P.device_ids[0] : 0; break;
            default: FL_FAIL(FL_ERR_BAD_ARGUMENT, "unknown tp mode %d", P.mode);
        }
        if (sh.rank < 0 || sh.rank >= tp) FL_FAIL(FL_ERR_BAD_ARGUMENT, "tp_rank %d out of range", sh.rank);
        if (sh.device < 0 || sh.device >= ndev) FL_FAIL(FL_ERR_NO_DEVICE, "device %d not present (%d visible)", sh.device, ndev);
        sh.Hs = D.H / tp; sh.Hkvs = D.Hkv / tp; sh.Is = D.inter / tp; sh.Ip = (sh.Is + 15) / 16 * 16;
        sh.Vs = m->vocab_parallel ? D.V / tp : D.V; sh.v0 = m->vocab_parallel ? sh.Vs * sh.rank : 0;
        FL_HIP(hipSetDevice(sh.device));
        if (P.mode == FL_TP_EMULATED && i > 0) sh.stream = m->shards[0].stream;     // one stream: sequential
        else FL_HIP(hipStreamCreateWithFlags(&sh.stream, hipStreamNonBlocking));
    }
    {   // is it a gfx950?
        hipDeviceProp_t prop;
        FL_HIP(hipGetDeviceProperties(&prop, m->shards[0].device));
        if (!strstr(prop.gcnArchName, "gfx950") && !tune(TK_ALLOW_ANY_ARCH))
            FL_FAIL(FL_ERR_NO_DEVICE, "device is %s; this library is built for gfx950 only", prop.gcnArchName);
    }

    Builder B; B.m = m.get();
    bool device_sources = false;
    for (size_t i = 0; i < n; i++) {
        if (!tensors[i].name) FL_FAIL(FL_ERR_BAD_ARGUMENT, "tensor %zu has no name", i);
        B.map[tensors[i].name] = &tensors[i];
        device_sources = device_sources || tensors[i].device >= 0;
    }
    if (device_sources) {
        // source tensors already in HBM may still be in flight on the caller's streams (a framework's generator or
        // loader); the conversion kernels run on this model's own streams, so wait for the devices first
        for (auto &sh : m->shards) { FL_HIP(hipSetDevice(sh.device)); FL_HIP(hipDeviceSynchronize()); }
    }
    FL_TRY(build_weights(B));
    if (decode_weights == FL_WEIGHTS_E4M3_ROW) FL_TRY(quantize_weights(m.get()));
    FL_TRY(build_rope(m.get()));
    for (auto &sh : m->shards) {
        FL_HIP(hipSetDevice(sh.device));
        FL_TRY(alloc_scratch(m.get(), sh, sh.dec, 1));
        FL_TRY(dev_alloc(sh.allocs, (void **)&sh.logits_local, (size_t)sh.Vs * 4, &m->hbm_bytes));
        FL_TRY(dev_alloc(sh.allocs, (void **)&sh.logits_full, (size_t)D.V * 4, &m->hbm_bytes));
        FL_TRY(dev_alloc(sh.allocs, (void **)&sh.amax, sizeof(ArgmaxCand) * kMaxArgmaxCand, &m->hbm_bytes));
        // the persistent decode engine's granule edges and tag epoch (k_engine.hip); tags never repeat, so they are zeroed once
        if (compute_dtype == FL_DTYPE_BF16 && engine_shape_ok(D.h, sh.Hs * D.d, sh.Ip, sh.Vs) && D.L <= 63) {
            const size_t ne[3] = {(size_t)D.h, (size_t)sh.Ip / 2, (size_t)D.h};
            for (int e = 0; e < 3; e++) {
                FL_TRY(dev_alloc(sh.allocs, (void **)&sh.eng_edge[e], ne[e] * 8, &m->hbm_bytes));
                FL_HIP(hipMemsetAsync(sh.eng_edge[e], 0, ne[e] * 8, sh.stream));
            }
            FL_TRY(dev_alloc(sh.allocs, (void **)&sh.eng_epoch, 16, &m->hbm_bytes));
            FL_HIP(hipMemsetAsync(sh.eng_epoch, 0, 16, sh.stream));
        }
    }
    FL_HIP(hipSetDevice(m->shards[0].device));
    FL_HIP(hipHostMalloc((void **)&m->host_logits, (size_t)D.V * 4, hipHostMallocDefault));
    FL_HIP(hipHostMalloc((void **)&m->host_tokens, kOutTokensCap * 4, hipHostMallocDefault));
    FL_HIP(hipHostMalloc((void **)&m->host_state, sizeof(StepState), hipHostMallocDefault));
#ifdef FL_EXPERIMENTAL
    m->engine = tune(TK_ENGINE);                  // persistent decode engine (k_engine.hip): 1 = wherever it runs (opt-in: it measured slower)
    m->fuse_oproj = tune(TK_FUSE_OPROJ);          // 0.0-1.5 % at best (profiles/r02/README.md): off unless asked for; -1 = where it pays most
#else
    m->engine = 0; m->fuse_oproj = 0;             // measured losers live in the EXPERIMENTAL build only (Makefile)
#endif

    // communicators
    if (tp > 1 && P.mode == FL_TP_SINGLE_PROCESS) {
        // One process drives all tp GPUs (the reference's process model).  The inboxes of the one-shot collectives
        // are then plain peer pointers -- no IPC -- and because those collectives synchronise through memory, every
        // shard's decode step is an independent hipGraph on its own stream.  RCCL (group calls) carries the large
        // prefill collectives; it refuses two ranks on one device, so a group with repeated device ids (a one-GPU
        // rehearsal) runs everything one-shot.
        if (tp > FL_MAX_TP) FL_FAIL(FL_ERR_UNSUPPORTED, "tp_size %d > %d", tp, FL_MAX_TP);
        std::vector<int> devs; for (auto &sh : m->shards) devs.push_back(sh.device);
        bool distinct = true;
        for (int i = 0; i < tp; i++) for (int j = 0; j < i; j++) distinct = distinct && devs[i] != devs[j];
        if (distinct) {
            std::vector<ncclComm_t> comms(tp);
            FL_NCCL(ncclCommInitAll(comms.data(), tp, devs.data()));
            for (int i = 0; i < tp; i++) m->shards[i].comm = comms[i];
        }
        if (tune(TK_ONESHOT) || !distinct) {
            bool ok = true;
            for (int i = 0; i < tp && ok; i++) ok = comm_alloc(m.get(), m->shards[i]) == FL_OK;
            for (int i = 0; i < tp && ok; i++) {
                (void)hipSetDevice(devs[i]);
                for (int j = 0; j < tp && ok; j++) {
                    if (devs[j] == devs[i]) continue;
                    const hipError_t e = hipDeviceEnablePeerAccess(devs[j], 0);
                    if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) ok = false;
                    (void)hipGetLastError();
                }
            }
            if (ok) {
                for (int i = 0; i < tp; i++) {
                    for (int r = 0; r < tp; r++) comm_set_entry(m->shards[i].pc, r, m->shards[r].pc.local);
                    m->shards[i].pc.connected = true;
                    m->shards[i].pc.shares_device = !distinct;
                    FL_TRY(comm_ll_publish(m.get(), m->shards[i]));
                }
            } else if (!distinct) {
                FL_FAIL(FL_ERR_RCCL, "cannot connect the shards of a single-device tensor-parallel group");
            }
        }
    } else if (tp > 1 && P.mode == FL_TP_MULTI_PROCESS) {
        // Small collectives (decode) go over peer-mapped inboxes; RCCL carries the large prefill ones.
        // Without a unique_id there is no RCCL communicator: the host must connect the inboxes itself
        // (fl_comm_ipc_export / fl_comm_ipc_connect) and every collective takes the one-shot path.
        if (tp > FL_MAX_TP) FL_FAIL(FL_ERR_UNSUPPORTED, "tp_size %d > %d", tp, FL_MAX_TP);
        FL_TRY(comm_alloc(m.get(), m->shards[0]));
        if (P.unique_id) {
            ncclUniqueId id; memcpy(&id, P.unique_id, sizeof id);
            FL_HIP(hipSetDevice(m->shards[0].device));
            FL_NCCL(ncclCommInitRank(&m->shards[0].comm, tp, id, P.tp_rank));
            if (tune(TK_ONESHOT)) FL_TRY(comm_bootstrap_over_rccl(m.get()));
        } else if (tune(TK_DEBUG_TP_LOOPBACK)) {
            FL_TRY(comm_connect_loopback(m.get()));
        }
    } else if (tp > 1 && P.mode == FL_TP_EMULATED) {
        FL_HIP(hipMalloc((void **)&m->emu_ptrs, sizeof(float *) * tp * 2));
    } else if (tp > 1) {
        FL_FAIL(FL_ERR_BAD_ARGUMENT, "tp_size %d needs a tensor-parallel mode", tp);
    } else if (tune(TK_DEBUG_RCCL_SELF)) {
        // single-GPU rehearsal of the RCCL plumbing: a 1-rank communicator whose all-reduce is the
        // identity, issued at the two real call sites (after o_proj and down_proj) on the compute stream
        ncclUniqueId id;
        FL_NCCL(ncclGetUniqueId(&id));
        FL_HIP(hipSetDevice(m->shards[0].device));
        FL_NCCL(ncclCommInitRank(&m->shards[0].comm, 1, id, 0));
        m->use_graph = tune(TK_GRAPH) > 0;              // eager unless graph capture of RCCL is asked for
        if (tune(TK_ONESHOT)) {                 // ... and of the inbox bootstrap: a group of one
            FL_TRY(comm_alloc(m.get(), m->shards[0]));
            FL_TRY(comm_bootstrap_over_rccl(m.get()));
        }
    }
    *out = m.release();
    return FL_OK;
}

}  // namespace fl
