// encoder.hip -- fl_encoder: weights, workspace and the forward of the BERT / MiniLM encoder (the reference's MiniLMModel,
// src/models/embeddings.rs:245-394, and EmbeddingModel::embed, :396-447) over a packed batch of sequences.  One GPU, one stream, no
// graph capture (the shapes change with every call).  A layer is four projections through the planner of k_linear.hip -- Q | K | V as
// one [3h, h] matrix, attention output, intermediate, output -- each left as fp32 (split-K slabs where the planner wants them) with
// its bias added by the launch that consumes it (k_encoder.hip).
#include <algorithm>
#include <memory>
#include <string>
#include <unordered_map>

#include "encoder.h"
#include "model.h"     // require_device

namespace fl {

// K slabs a projection of T rows may leave (the consumers sum them): short and mid-size batches are weight streams that gain from
// them; above, the row tiles fill the chip.  `y` is sized for the same rule.
static int enc_split_cap(int64_t T) { return T <= 1 ? 1 : T <= 1024 ? 4 : 1; }

Encoder::~Encoder() {
    (void)hipSetDevice(device);
    if (stream) {
        (void)hipStreamSynchronize(stream);
        gemm_8p_release_stream(stream);
        gemm_h4_release_stream(stream);
        gemm_skf_release_stream(stream);
        (void)hipStreamDestroy(stream);
    }
    for (void *p : allocs) (void)hipFree(p);
}

static int enc_alloc(Encoder *e, void **p, size_t bytes) {
    if (bytes == 0) bytes = 16;
    const hipError_t err = hipMalloc(p, bytes);
    if (err == hipErrorOutOfMemory) { (void)hipGetLastError(); FL_FAIL(FL_ERR_OOM, "out of HBM: hipMalloc of %zu bytes failed", bytes); }
    FL_HIP(err);
    e->allocs.push_back(*p);
    e->hbm_bytes += (int64_t)bytes;
    return FL_OK;
}

namespace {
struct EncBuilder {
    Encoder *e;
    std::unordered_map<std::string, const fl_tensor *> map;
    void *stage = nullptr; size_t stage_cap = 0;
    ~EncBuilder() { if (stage) (void)hipFree(stage); }

    // rows < 0: any positive row count (the token-type table, of which row 0 is used)
    int want(const std::string &name, int64_t R, int64_t C, const fl_tensor **out) const {
        auto it = map.find(name);
        if (it == map.end()) FL_FAIL(FL_ERR_MISSING_TENSOR, "cannot find tensor %s", name.c_str());
        const fl_tensor *t = it->second;
        if (t->dtype < FL_DTYPE_F32 || t->dtype > FL_DTYPE_F16) FL_FAIL(FL_ERR_UNSUPPORTED, "tensor %s: unsupported dtype %d", name.c_str(), t->dtype);
        const bool ok = C == 1 ? (t->ndim == 1 && t->shape[0] == R) : (t->ndim == 2 && (R < 0 ? t->shape[0] >= 1 : t->shape[0] == R) && t->shape[1] == C);
        if (!ok) FL_FAIL(FL_ERR_SHAPE_MISMATCH, "shape mismatch for %s: expected [%lld,%lld]", name.c_str(), (long long)R, (long long)C);
        if (!t->data) FL_FAIL(FL_ERR_BAD_ARGUMENT, "tensor %s has null data", name.c_str());
        *out = t;
        return FL_OK;
    }
    // the source on the encoder's device (host tensors and other devices' go through one reused staging buffer)
    int on_device(const fl_tensor &t, size_t elems, const void **out) {
        if (t.device == e->device) { *out = t.data; return FL_OK; }
        const size_t bytes = elems * (t.dtype == FL_DTYPE_F32 ? 4 : 2);
        if (bytes > stage_cap) {
            if (stage) { FL_HIP(hipFree(stage)); stage = nullptr; stage_cap = 0; }
            FL_HIP(hipMalloc(&stage, bytes));
            stage_cap = bytes;
        }
        FL_HIP(hipMemcpy(stage, t.data, bytes, hipMemcpyDefault));
        *out = stage;
        return FL_OK;
    }
    // rows [0, R) x C of `name` -> dst rows [row0, row0 + R) of a matrix with C columns, in dst_dtype
    int matrix(const std::string &name, int64_t R, int64_t C, int dst_dtype, void *dst, int64_t row0, int64_t rows_used = -1) {
        const fl_tensor *t = nullptr;
        FL_TRY(want(name, R, C, &t));
        const int64_t rows = rows_used > 0 ? rows_used : R;
        const void *src = nullptr;
        FL_TRY(on_device(*t, (size_t)rows * C, &src));
        Launcher L; L.stream = e->stream;
        FL_TRY(launch_convert_slice(L, t->dtype, src, C, 0, 0, rows, C, dst_dtype, dst, C, row0, 0));
        FL_HIP(hipStreamSynchronize(e->stream));            // the staging buffer is reused by the next tensor
        return FL_OK;
    }
    int vec(const std::string &name, int64_t n, float *dst) {
        const fl_tensor *t = nullptr;
        FL_TRY(want(name, n, 1, &t));
        const void *src = nullptr;
        FL_TRY(on_device(*t, (size_t)n, &src));
        Launcher L; L.stream = e->stream;
        FL_TRY(launch_convert_vec_f32(L, t->dtype, src, 0, n, dst));
        FL_HIP(hipStreamSynchronize(e->stream));
        return FL_OK;
    }
};
}  // namespace

int encoder_create(const fl_encoder_config *cfg, const fl_tensor *tensors, size_t n, int compute_dtype, int device, Encoder **out) {
    if (!out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_encoder_create: null out");
    *out = nullptr;
    if (!cfg) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_encoder_create: null config");
    if (cfg->struct_size != sizeof(fl_encoder_config))
        FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_encoder_config.struct_size is %u, this library's is %zu", cfg->struct_size, sizeof(fl_encoder_config));
    if (!tensors && n) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null tensors");
    if (cfg->activation != FL_ACT_GELU_TANH && cfg->activation != FL_ACT_GELU_ERF) FL_FAIL(FL_ERR_BAD_ARGUMENT, "unknown activation %d (fl_activation)", cfg->activation);
    if (compute_dtype != FL_DTYPE_BF16 && compute_dtype != FL_DTYPE_F32) FL_FAIL(FL_ERR_BAD_ARGUMENT, "compute dtype must be FL_DTYPE_F32 or FL_DTYPE_BF16");
    if (device < 0) FL_FAIL(FL_ERR_BAD_ARGUMENT, "negative device ordinal");
    const int64_t h = cfg->hidden_size, I = cfg->intermediate_size, Ly = cfg->num_hidden_layers, H = cfg->num_attention_heads,
                  P = cfg->max_position_embeddings, V = cfg->vocab_size;
    if (h <= 0 || I <= 0 || Ly <= 0 || H <= 0 || P <= 0 || V <= 0 || cfg->max_batch_tokens < 0 || !(cfg->layer_norm_eps >= 0.0))
        FL_FAIL(FL_ERR_BAD_CONFIG, "encoder config: every size must be positive (hidden %lld, intermediate %lld, layers %lld, heads %lld, positions %lld, vocabulary %lld)",
                (long long)h, (long long)I, (long long)Ly, (long long)H, (long long)P, (long long)V);
    if (h % H) FL_FAIL(FL_ERR_BAD_CONFIG, "hidden_size %lld is not divisible by num_attention_heads %lld", (long long)h, (long long)H);
    const int64_t d = h / H;
    if (!encoder_attention_supported(d)) FL_FAIL(FL_ERR_UNSUPPORTED, "encoder head_dim %lld not supported (32: MiniLM-L6 / L12; 64: BERT-base / large shapes)", (long long)d);
    // (hidden_size = heads x 32 or heads x 64 is a multiple of 8 by now)
    if (I % 8) FL_FAIL(FL_ERR_UNSUPPORTED, "intermediate_size %lld must be a multiple of 8 (16-byte rows)", (long long)I);
    if (cfg->_pad || cfg->_reserved[0] || cfg->_reserved[1]) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_encoder_config: _pad and _reserved must be 0");
    const int64_t max_T = cfg->max_batch_tokens ? cfg->max_batch_tokens : 4096;
    if (max_T > (1 << 20) || P > (1 << 18) || V > ((int64_t)1 << 31) - 1 || H > 65535)
        FL_FAIL(FL_ERR_UNSUPPORTED, "encoder config beyond the kernels' index range (max_batch_tokens <= 2^20, max_position_embeddings <= 2^18)");

    int ndev = 0;
    FL_TRY(require_device(&ndev));
    if (device >= ndev) FL_FAIL(FL_ERR_NO_DEVICE, "device %d not present (%d visible)", device, ndev);
    {
        hipDeviceProp_t prop;
        FL_HIP(hipGetDeviceProperties(&prop, device));
        if (!strstr(prop.gcnArchName, "gfx950") && !tune(TK_ALLOW_ANY_ARCH))
            FL_FAIL(FL_ERR_NO_DEVICE, "device is %s; this library is built for gfx950 only", prop.gcnArchName);
    }

    std::unique_ptr<Encoder> e(new Encoder());
    e->device = device; e->dtype = compute_dtype; e->act = cfg->activation == FL_ACT_GELU_ERF ? ENC_ACT_GELU_ERF : ENC_ACT_GELU_TANH;
    e->h = h; e->inter = I; e->L = Ly; e->H = H; e->d = d; e->P = P; e->V = V; e->max_T = max_T; e->eps = (float)cfg->layer_norm_eps;
    FL_HIP(hipSetDevice(device));
    FL_HIP(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));

    EncBuilder B; B.e = e.get();
    bool device_sources = false;
    for (size_t i = 0; i < n; i++) {
        if (!tensors[i].name) FL_FAIL(FL_ERR_BAD_ARGUMENT, "tensor %zu has no name", i);
        B.map[tensors[i].name] = &tensors[i];
        device_sources = device_sources || tensors[i].device >= 0;
    }
    if (device_sources) FL_HIP(hipDeviceSynchronize());     // sources in HBM may still be in flight on the caller's streams

    const int wdt = compute_dtype;
    const size_t es = e->esize();
    Encoder *E = e.get();
    FL_TRY(enc_alloc(E, &e->word, (size_t)V * h * es));
    FL_TRY(enc_alloc(E, &e->pos, (size_t)P * h * es));
    FL_TRY(enc_alloc(E, (void **)&e->lnw, (size_t)h * 4));
    FL_TRY(enc_alloc(E, (void **)&e->lnb, (size_t)h * 4));
    FL_TRY(B.matrix("embeddings.word_embeddings.weight", V, h, wdt, e->word, 0));
    FL_TRY(B.matrix("embeddings.position_embeddings.weight", P, h, wdt, e->pos, 0));
    FL_TRY(B.vec("embeddings.LayerNorm.weight", h, e->lnw));
    FL_TRY(B.vec("embeddings.LayerNorm.bias", h, e->lnb));
    if (cfg->add_token_type0) {
        FL_TRY(enc_alloc(E, &e->tt0, (size_t)h * es));
        FL_TRY(B.matrix("embeddings.token_type_embeddings.weight", -1, h, wdt, e->tt0, 0, 1));
    }
    e->layers.resize((size_t)Ly);
    for (int64_t l = 0; l < Ly; l++) {
        EncLayerW &w = e->layers[(size_t)l];
        const std::string p = "encoder.layer." + std::to_string(l) + ".";
        FL_TRY(enc_alloc(E, &w.wqkv, (size_t)3 * h * h * es));
        FL_TRY(enc_alloc(E, (void **)&w.bqkv, (size_t)3 * h * 4));
        FL_TRY(enc_alloc(E, &w.wo, (size_t)h * h * es));
        FL_TRY(enc_alloc(E, &w.wi, (size_t)I * h * es));
        FL_TRY(enc_alloc(E, &w.wout, (size_t)h * I * es));
        float **vecs[] = {&w.bo, &w.ln1w, &w.ln1b, &w.bout, &w.ln2w, &w.ln2b};
        for (float **v : vecs) FL_TRY(enc_alloc(E, (void **)v, (size_t)h * 4));
        FL_TRY(enc_alloc(E, (void **)&w.bi, (size_t)I * 4));
        const char *qkv[3] = {"attention.self.query", "attention.self.key", "attention.self.value"};
        for (int i = 0; i < 3; i++) {
            FL_TRY(B.matrix(p + qkv[i] + ".weight", h, h, wdt, w.wqkv, i * h));
            FL_TRY(B.vec(p + qkv[i] + ".bias", h, w.bqkv + i * h));
        }
        FL_TRY(B.matrix(p + "attention.output.dense.weight", h, h, wdt, w.wo, 0));
        FL_TRY(B.vec(p + "attention.output.dense.bias", h, w.bo));
        FL_TRY(B.vec(p + "attention.output.LayerNorm.weight", h, w.ln1w));
        FL_TRY(B.vec(p + "attention.output.LayerNorm.bias", h, w.ln1b));
        FL_TRY(B.matrix(p + "intermediate.dense.weight", I, h, wdt, w.wi, 0));
        FL_TRY(B.vec(p + "intermediate.dense.bias", I, w.bi));
        FL_TRY(B.matrix(p + "output.dense.weight", h, I, wdt, w.wout, 0));
        FL_TRY(B.vec(p + "output.dense.bias", h, w.bout));
        FL_TRY(B.vec(p + "output.LayerNorm.weight", h, w.ln2w));
        FL_TRY(B.vec(p + "output.LayerNorm.bias", h, w.ln2b));
    }

    // workspace
    const int64_t T = max_T, wide = std::max<int64_t>(3 * h, I);
    e->slab_rows = std::max<int64_t>(T, std::min<int64_t>(T, 1024) * enc_split_cap(std::min<int64_t>(T, 1024)));
    FL_TRY(enc_alloc(E, (void **)&e->x_res, (size_t)T * h * 4));
    FL_TRY(enc_alloc(E, &e->xn, (size_t)T * h * es));
    FL_TRY(enc_alloc(E, (void **)&e->y, (size_t)e->slab_rows * wide * 4));
    FL_TRY(enc_alloc(E, &e->qkv, (size_t)T * 3 * h * es));
    FL_TRY(enc_alloc(E, &e->ao, (size_t)T * h * es));
    FL_TRY(enc_alloc(E, &e->gelu, (size_t)T * I * es));
    FL_TRY(enc_alloc(E, (void **)&e->pooled, (size_t)T * h * 4));
    FL_TRY(enc_alloc(E, (void **)&e->ids, (size_t)T * 4));
    FL_TRY(enc_alloc(E, (void **)&e->row_seq, (size_t)T * 4));
    FL_TRY(enc_alloc(E, (void **)&e->offsets, (size_t)(T + 1) * 4));
    FL_HIP(hipStreamSynchronize(e->stream));
    *out = e.release();
    return FL_OK;
}

int encoder_check_offsets(const size_t *offsets, size_t n_seq, int64_t max_len, int64_t max_total, int64_t *total_out, int64_t *longest_out) {
    if (!offsets || n_seq == 0) FL_FAIL(FL_ERR_BAD_ARGUMENT, "encoder: null offsets / no sequence");
    if (offsets[0] != 0) FL_FAIL(FL_ERR_BAD_ARGUMENT, "encoder: offsets[0] must be 0");
    int64_t longest = 0;
    for (size_t s = 0; s < n_seq; s++) {
        if (offsets[s + 1] < offsets[s]) FL_FAIL(FL_ERR_BAD_ARGUMENT, "encoder: offsets decrease at sequence %zu", s);
        if (offsets[s + 1] == offsets[s]) FL_FAIL(FL_ERR_BAD_ARGUMENT, "encoder: sequence %zu is empty (the mean over no token is undefined)", s);
        const size_t len = offsets[s + 1] - offsets[s];
        if (max_len > 0 && len > (size_t)max_len) FL_FAIL(FL_ERR_SEQ_OVERFLOW, "encoder: sequence %zu has %zu tokens, max_position_embeddings is %lld", s, len, (long long)max_len);
        if (offsets[s + 1] > (size_t)max_total) FL_FAIL(FL_ERR_SEQ_OVERFLOW, "encoder: more than %lld tokens in one call (max_batch_tokens)", (long long)max_total);
        longest = std::max<int64_t>(longest, (int64_t)len);
    }
    *total_out = (int64_t)offsets[n_seq];
    *longest_out = longest;
    return FL_OK;
}

// one projection through the planner: fp32 output in *n_split slabs of [T][N] in e->y, no bias (the consumer adds it)
static int enc_linear(Encoder *e, Launcher &L, const void *W, const void *x, int64_t T, int64_t N, int64_t K, int *n_split) {
    const int cap = enc_split_cap(T);
    const LinearPlan p = plan_linear(e->dtype, T, N, K, EPI_F32, 1, cap, false, true, false);
    if (p.n_split > cap || (int64_t)p.n_split * T > e->slab_rows) FL_FAIL(FL_ERR_UNSUPPORTED, "encoder: the planner asked for %d K slabs at %lld rows (workspace holds %d)", p.n_split, (long long)T, cap);
    *n_split = p.n_split;
    return launch_plan(L, p, e->dtype, W, x, nullptr, e->y, T, N, K, EPI_F32, nullptr);
}

static int encoder_enqueue(Encoder *e, int64_t n_seq, int64_t T, int64_t longest, float *hidden_out, float *embed_out);

int encoder_run(Encoder *e, const uint32_t *ids, const size_t *offsets, size_t n_seq, float *hidden_out, float *embed_out) {
    if (!e) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null encoder");
    if (!ids || (!hidden_out && !embed_out)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "encoder: null ids / out");
    int64_t T = 0, longest = 0;
    FL_TRY(encoder_check_offsets(offsets, n_seq, e->P, e->max_T, &T, &longest));
    for (int64_t t = 0; t < T; t++)
        if ((int64_t)ids[t] >= e->V) FL_FAIL(FL_ERR_BAD_ARGUMENT, "encoder: token id %u at %lld is outside the vocabulary (%lld)", ids[t], (long long)t, (long long)e->V);
    std::vector<int32_t> row_seq((size_t)T), offs(n_seq + 1);
    for (size_t s = 0; s <= n_seq; s++) offs[s] = (int32_t)offsets[s];
    for (size_t s = 0; s < n_seq; s++)
        for (size_t r = offsets[s]; r < offsets[s + 1]; r++) row_seq[r] = (int32_t)s;

    std::lock_guard<std::mutex> lock(e->mu);
    FL_HIP(hipSetDevice(e->device));
    hipStream_t st = e->stream;
    FL_HIP(hipMemcpyAsync(e->ids, ids, (size_t)T * 4, hipMemcpyHostToDevice, st));
    FL_HIP(hipMemcpyAsync(e->row_seq, row_seq.data(), (size_t)T * 4, hipMemcpyHostToDevice, st));
    FL_HIP(hipMemcpyAsync(e->offsets, offs.data(), (n_seq + 1) * 4, hipMemcpyHostToDevice, st));
    FL_HIP(hipStreamSynchronize(st));                       // the host vectors above are pageable and go out of scope
    // a launch that fails part-way leaves earlier work queued: wait for it before the error goes back, so that the next call finds an idle stream
    const int rc = encoder_enqueue(e, (int64_t)n_seq, T, longest, hidden_out, embed_out);
    const hipError_t se = hipStreamSynchronize(st);
    if (rc != FL_OK) { (void)hipGetLastError(); return rc; }
    FL_HIP(se);
    return FL_OK;
}

static int encoder_enqueue(Encoder *e, int64_t n_seq, int64_t T, int64_t longest, float *hidden_out, float *embed_out) {
    hipStream_t st = e->stream;
    Launcher L; L.stream = st;
    const int dt = e->dtype;
    const int64_t h = e->h, I = e->inter;
    const size_t es = e->esize();
    const float scale = 1.0f / sqrtf((float)e->d);
    // embeddings.LayerNorm: eps hard-wired to 1e-12 (embeddings.rs:317), not the config's
    FL_TRY(launch_encoder_embed_ln(L, dt, e->word, e->pos, e->tt0, e->ids, e->row_seq, e->offsets, e->lnw, e->lnb, 1e-12f, e->x_res, e->xn, T, h));
    for (const EncLayerW &w : e->layers) {
        int ns = 1;
        FL_TRY(enc_linear(e, L, w.wqkv, e->xn, T, 3 * h, h, &ns));
        FL_TRY(launch_encoder_bias_act(L, dt, e->y, ns, T * 3 * h, w.bqkv, ENC_ACT_NONE, e->qkv, T, 3 * h));
        const char *qp = (const char *)e->qkv;
        FL_TRY(launch_encoder_attention(L, dt, qp, qp + (size_t)h * es, qp + (size_t)2 * h * es, 3 * h, e->offsets, n_seq, longest, T, e->H,
                                        e->d, scale, e->ao));
        FL_TRY(enc_linear(e, L, w.wo, e->ao, T, h, h, &ns));
        FL_TRY(launch_encoder_add_ln(L, dt, e->x_res, e->y, ns, T * h, w.bo, w.ln1w, w.ln1b, e->eps, e->xn, T, h));
        FL_TRY(enc_linear(e, L, w.wi, e->xn, T, I, h, &ns));
        FL_TRY(launch_encoder_bias_act(L, dt, e->y, ns, T * I, w.bi, e->act, e->gelu, T, I));
        FL_TRY(enc_linear(e, L, w.wout, e->gelu, T, h, I, &ns));
        FL_TRY(launch_encoder_add_ln(L, dt, e->x_res, e->y, ns, T * h, w.bout, w.ln2w, w.ln2b, e->eps, e->xn, T, h));
    }
    if (hidden_out) {
        FL_HIP(hipMemcpyAsync(hidden_out, e->x_res, (size_t)T * h * 4, hipMemcpyDeviceToHost, st));
    } else {
        FL_TRY(launch_encoder_pool_l2(L, e->x_res, e->offsets, n_seq, h, e->pooled));
        FL_HIP(hipMemcpyAsync(embed_out, e->pooled, (size_t)n_seq * h * 4, hipMemcpyDeviceToHost, st));
    }
    return FL_OK;
}

}  // namespace fl
