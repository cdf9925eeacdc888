// api_ops.hip -- the fl_op_* entry points: one kernel (or one launch sequence) on host arrays, for the tests and tools/.  Each is its
// argument checks, then an OpScope (device 0, a stream, the device buffers), the launches, and the download of the result.
#include <algorithm>
#include <memory>
#include <vector>

#include "api_internal.h"
#include "encoder.h"

using namespace fl;

namespace {

// What an op body runs in: device 0, a stream of its own, every device allocation made through it and the event pair of a timed run.
// Leaving the scope -- on an error return too -- waits for the stream before anything it may still be using is freed.
struct OpScope {
    hipStream_t s = 0; hipEvent_t e0 = 0, e1 = 0;
    std::vector<void *> p;
    Launcher L;
    int begin() { FL_TRY(require_device()); FL_HIP(hipSetDevice(0)); FL_HIP(hipStreamCreate(&s)); L.stream = s; return FL_OK; }
    ~OpScope() {
        // the split-K workspaces the GEMMs keep per stream go before the stream does (no-ops for a stream they never saw)
        if (s) { (void)hipStreamSynchronize(s); gemm_8p_release_stream(s); gemm_h4_release_stream(s); gemm_skf_release_stream(s); }
        for (void *x : p) (void)hipFree(x);
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        if (s) (void)hipStreamDestroy(s);
    }
    template <typename T> int alloc(T **out, size_t bytes) { *out = nullptr; FL_HIP(hipMalloc((void **)out, bytes ? bytes : 4)); p.push_back(*out); return FL_OK; }
    template <typename T> int upload(T **out, const void *src, size_t bytes) { FL_TRY(alloc(out, bytes)); FL_HIP(hipMemcpy(*out, src, bytes, hipMemcpyHostToDevice)); return FL_OK; }
};

// The launches of an op that can be timed.  Always: run(0) once and a synchronise.  With iters > 0 and an ms_out, then: one warming
// launch per copy, and `iters` launches between two events; *ms_out = ms per launch.
// The timed launches rotate over `ncopy` copies of the op's working set (`bytes` each; copy 0 is the op's own, make(c) adds copy
// c >= 1, run(c) launches on copy c) that together exceed the 256 MiB Infinity Cache: in the forward pass a projection's weights
// always come from HBM, and a back-to-back replay on ONE copy would read them from the cache.  op_hot = 1: one copy (L2 + Infinity
// Cache); n > 1: n copies (past the L2s, inside the Infinity Cache when n x bytes < 256 MiB).
template <typename Make, typename Run>
int op_run(OpScope &B, size_t bytes, int iters, double *ms_out, Make make, Run run) {
    const bool timed = iters > 0 && ms_out;
    const int hot = tune(TK_OP_HOT);
    const int ncopy = !timed ? 1 : hot > 0 ? hot : (int)std::min<size_t>(24, std::max<size_t>(1, (640u << 20) / bytes + 1));
    for (int c = 1; c < ncopy; c++) FL_TRY(make(c));
    FL_TRY(run(0));
    FL_HIP(hipStreamSynchronize(B.s));
    if (!timed) return FL_OK;
    for (int c = 0; c < ncopy; c++) FL_TRY(run(c));   // warm
    FL_HIP(hipStreamSynchronize(B.s));
    FL_HIP(hipEventCreate(&B.e0)); FL_HIP(hipEventCreate(&B.e1));
    FL_HIP(hipEventRecord(B.e0, B.s));
    for (int i = 0; i < iters; i++) FL_TRY(run(i % ncopy));
    FL_HIP(hipEventRecord(B.e1, B.s));
    FL_HIP(hipEventSynchronize(B.e1));
    float ms = 0.f; FL_HIP(hipEventElapsedTime(&ms, B.e0, B.e1));
    *ms_out = ms / iters;
    return FL_OK;
}

// a launch's output, [rows][pitch] elements of `dtype` on the device: the first `cols` of every row, widened to fp32, to out [rows][cols]
int op_download(float *out, const void *dev, size_t rows, size_t cols, size_t pitch, int32_t dtype) {
    if (dtype != FL_DTYPE_BF16 && cols == pitch) { FL_HIP(hipMemcpy(out, dev, rows * cols * 4, hipMemcpyDeviceToHost)); return FL_OK; }
    const size_t es = dtype == FL_DTYPE_BF16 ? 2 : 4;
    std::vector<unsigned char> tmp(rows * pitch * es);
    FL_HIP(hipMemcpy(tmp.data(), dev, tmp.size(), hipMemcpyDeviceToHost));
    for (size_t r = 0; r < rows; r++)
        for (size_t j = 0; j < cols; j++) {
            const size_t idx = r * pitch + j;
            out[r * cols + j] = es == 2 ? bf16_bits_to_float(reinterpret_cast<bf16_t *>(tmp.data())[idx]) : reinterpret_cast<float *>(tmp.data())[idx];
        }
    return FL_OK;
}
int op_download(float *out, const void *dev, size_t n, int32_t dtype) { return op_download(out, dev, 1, n, n, dtype); }

// ---- the attention ops: the launches on caches built here in the model's layout -------------------------------------------------

// One sequence's K and V as cache_create lays them out: K [L][Hkv][sa][d]; V the same, or transposed [L][Hkv][d][sa] for the MFMA
// kernels.  Host rows [L][rows][Hkv*d]; every position >= rows holds `pad`.  E: the element's bit pattern (uint16_t / uint32_t).
template <typename E>
void attn_op_cache(std::vector<E> &kc, std::vector<E> &vc, const void *k, const void *v, int64_t L, int64_t rows, int64_t Hkv, int64_t sa,
                   int64_t d, bool v_transposed, E pad) {
    kc.assign((size_t)(L * Hkv * sa * d), pad); vc.assign((size_t)(L * Hkv * sa * d), pad);
    const E *kh = reinterpret_cast<const E *>(k), *vh = reinterpret_cast<const E *>(v);
    for (int64_t l = 0; l < L; l++)
        for (int64_t s = 0; s < rows; s++)
            for (int64_t h = 0; h < Hkv; h++)
                for (int64_t j = 0; j < d; j++) {
                    const size_t src = (size_t)(((l * rows + s) * Hkv + h) * d + j), head = (size_t)((l * Hkv + h) * sa * d);
                    kc[head + (size_t)(s * d + j)] = kh[src];
                    vc[head + (size_t)(v_transposed ? j * sa + s : s * d + j)] = vh[src];
                }
}

int attn_op_upload_cache(OpScope &B, void **kd, void **vd, int32_t dtype, const void *k, const void *v, int64_t L, int64_t rows, int64_t Hkv,
                         int64_t sa, int64_t d, bool v_transposed, float pad_value) {
    if (dtype == FL_DTYPE_BF16) {
        std::vector<uint16_t> kc, vc;
        attn_op_cache<uint16_t>(kc, vc, k, v, L, rows, Hkv, sa, d, v_transposed, float_to_bf16_bits_host(pad_value));
        FL_TRY(B.upload(kd, kc.data(), kc.size() * 2)); FL_TRY(B.upload(vd, vc.data(), vc.size() * 2));
    } else {
        union { float f; uint32_t u; } pv; pv.f = pad_value;
        std::vector<uint32_t> kc, vc;
        attn_op_cache<uint32_t>(kc, vc, k, v, L, rows, Hkv, sa, d, v_transposed, pv.u);
        FL_TRY(B.upload(kd, kc.data(), kc.size() * 4)); FL_TRY(B.upload(vd, vc.data(), vc.size() * 4));
    }
    return FL_OK;
}

// the split scratch of one cache, sized as cache_create sizes it
int attn_op_scratch(OpScope &B, float **pm, float **pl, float **po, unsigned **cnt, int64_t H, int64_t d, int nsplit) {
    FL_TRY(B.alloc(pm, (size_t)H * nsplit * 4)); FL_TRY(B.alloc(pl, (size_t)H * nsplit * 4));
    FL_TRY(B.alloc(po, (size_t)H * nsplit * d * 4)); FL_TRY(B.alloc(cnt, (size_t)H * 4));
    FL_HIP(hipMemset(*cnt, 0, (size_t)H * 4));
    return FL_OK;
}

// ---- the norm ops ---------------------------------------------------------------------------------------------------------------

static_assert(FL_LK_NONE == LK_NONE && FL_LK_GEMV == LK_GEMV && FL_LK_H4 == LK_H4 && FL_LK_W14 == LK_W14 && FL_LK_SKF == LK_SKF && FL_LK_DMA == LK_DMA &&
              FL_LK_SKINNY == LK_SKINNY && FL_LK_8P == LK_8P && FL_LK_8P_STREAMK == LK_8P_STREAMK && FL_LK_256 == LK_256 && FL_LK_128 == LK_128 &&
              FL_LK_4W_ROPE == LK_4W_ROPE && FL_LK_GENERIC == LK_GENERIC && FL_LK_F32_ROWS == LK_F32_ROWS && FL_LK_F32_MFMA == LK_F32_MFMA,
              "the header's FL_LK_* codes are kernels.h's LK_*");

// The device image of a host matrix w [N][K] of `dtype`: as it is, or (gate/up: rows gate | up in HF order) in the 16-interleaved
// layout with the pairs padded to whole groups of 16, as fl_op_linear lays it out.  *Nw: its rows; *Ip: the padded pair count.
int op_upload_matrix(OpScope &B, int32_t dtype, const void *w, int64_t N, int64_t K, int epi, void **wd, int64_t *Nw, int64_t *Ip) {
    const size_t es = dtype == FL_DTYPE_BF16 ? 2 : 4;
    const int64_t I = N / 2;
    *Ip = (I + 15) / 16 * 16;
    *Nw = epi == EPI_GATEUP ? 2 * *Ip : N;
    if (epi != EPI_GATEUP) return B.upload(wd, w, (size_t)N * K * es);
    void *ws;
    FL_TRY(B.upload(&ws, w, (size_t)N * K * es));
    FL_TRY(B.alloc(wd, (size_t)*Nw * K * es));
    FL_HIP(hipMemsetAsync(*wd, 0, (size_t)*Nw * K * es, B.s));
    FL_TRY(launch_convert_slice(B.L, dtype, ws, K, 0, 0, I, K, dtype, *wd, K, 0, 1));
    return launch_convert_slice(B.L, dtype, ws, K, I, 0, I, K, dtype, *wd, K, 0, 2);
}

// the fl_op_norm_linear checks that need no device
int norm_linear_check(const fl_norm_linear_args *a) {
    if (!a) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_norm_linear: null args");
    if (a->struct_size != sizeof(fl_norm_linear_args)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_norm_linear: struct_size %zu, expected %zu", a->struct_size, sizeof(fl_norm_linear_args));
    if (a->form < 0 || a->form > 3) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_norm_linear: form %d not in 0..3", a->form);
    if (a->dtype != FL_DTYPE_BF16 && a->dtype != FL_DTYPE_F32) FL_FAIL(FL_ERR_UNSUPPORTED, "dtype must be bf16 or f32");
    if (a->epilogue != EPI_F32 && a->epilogue != EPI_GATEUP) FL_FAIL(FL_ERR_BAD_ARGUMENT, "epilogue must be 0 or 1");
    if (a->pro != PRO_X && a->pro != PRO_NORM) FL_FAIL(FL_ERR_BAD_ARGUMENT, "pro must be 0 or 1");
    if (a->pro == PRO_X && a->form != 3) FL_FAIL(FL_ERR_BAD_ARGUMENT, "pro 0 (no norm) is the batched stream's (form 3)");
    if (!a->w || !a->y) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument (w, y)");
    if (a->T <= 0 || a->N <= 0 || a->K <= 0 || a->K % 8 || a->N > (1 << 24)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "bad shape (K must be a multiple of 8)");
    if (a->epilogue == EPI_GATEUP && ((a->N % 2) || a->bias)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "gate/up needs an even row count and takes no bias");
    if (a->repeat < 1 || a->repeat > 8) FL_FAIL(FL_ERR_BAD_ARGUMENT, "repeat %d not in 1..8", a->repeat);
    if (a->pro == PRO_NORM) {
        if (!a->norm_w) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null norm_w");
        if (a->n_slab < 0 || a->n_slab > 64 || (a->n_slab > 0) != (a->delta != nullptr)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "n_slab 0..64, with delta exactly when it is not 0");
        if (a->embed) {
            if (a->x_res || a->delta || !a->tokens || a->vocab < 1) FL_FAIL(FL_ERR_BAD_ARGUMENT, "embed takes tokens and a vocab size, and neither x_res nor delta");
            for (int64_t t = 0; t < a->T; t++)
                if ((int64_t)a->tokens[t] >= a->vocab) FL_FAIL(FL_ERR_BAD_ARGUMENT, "tokens[%lld] = %u is not below vocab %lld", (long long)t, a->tokens[t], (long long)a->vocab);
        } else if (!a->x_res) {
            FL_FAIL(FL_ERR_BAD_ARGUMENT, "null x_res (and no embed)");
        }
    } else if (!a->x) {
        FL_FAIL(FL_ERR_BAD_ARGUMENT, "null x");
    }
    const int64_t Nw = a->epilogue == EPI_GATEUP ? (a->N / 2 + 15) / 16 * 32 : a->N;
    if (a->form == 1) {
        if (a->T != 1) FL_FAIL(FL_ERR_BAD_ARGUMENT, "form 1: the single-sequence stream takes one row");
        if (!gemv_norm_supported(a->dtype, Nw, a->K)) FL_FAIL(FL_ERR_UNSUPPORTED, "form 1: the norm prologue needs K <= 6144");
    } else if (a->form == 2) {
        if (a->T != 1) FL_FAIL(FL_ERR_BAD_ARGUMENT, "form 2: the single-sequence stream takes one row");
        if (!a->w_scale) FL_FAIL(FL_ERR_BAD_ARGUMENT, "form 2: null w_scale");
        if (a->dtype != FL_DTYPE_BF16 || a->n_slab > 1) FL_FAIL(FL_ERR_UNSUPPORTED, "form 2: bf16 activations, at most one delta vector");
        if (!gemv_w8_norm_supported(Nw, a->K)) FL_FAIL(FL_ERR_UNSUPPORTED, "form 2: K a multiple of 16, at most 6144");
    } else if (a->form == 3) {
        if (a->T > 8) FL_FAIL(FL_ERR_BAD_ARGUMENT, "form 3: at most 8 rows");
        if (a->dtype != FL_DTYPE_BF16) FL_FAIL(FL_ERR_UNSUPPORTED, "form 3: bf16");
    }
    return FL_OK;
}

// ---- the RoPE + KV-append ops: what fl_op_rope_kv and fl_op_qkv_rope share ---------------------------------------------------------

// the checks of an fl_rope_seqs that need no device; *rows_out: the rows of the call
int rope_seqs_check(const char *who, const fl_rope_seqs &q, int32_t dtype, int64_t H, int64_t Hkv, int64_t d, int64_t max_pos, const float *cos_tab,
                    const float *sin_tab, const void *q_out, int64_t *rows_out) {
    if (dtype != FL_DTYPE_BF16 && dtype != FL_DTYPE_F32) FL_FAIL(FL_ERR_UNSUPPORTED, "%s: dtype must be bf16 or f32", who);
    if (H < 1 || Hkv < 1 || H > 1024 || H % Hkv != 0) FL_FAIL(FL_ERR_BAD_ARGUMENT, "%s: bad head counts (H %lld a multiple of Hkv %lld)", who, (long long)H, (long long)Hkv);
    if (d < 2 || d > 1024 || d % 2) FL_FAIL(FL_ERR_BAD_ARGUMENT, "%s: head_dim %lld must be even (2..1024)", who, (long long)d);
    if (max_pos < 1 || max_pos > (1 << 24) || !cos_tab || !sin_tab) FL_FAIL(FL_ERR_BAD_ARGUMENT, "%s: cos_tab / sin_tab [max_pos][d / 2], 1 <= max_pos <= 2^24", who);
    if (!q_out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "%s: null q_out", who);
    if (q.n_seq < 1 || q.n_seq > 1024) FL_FAIL(FL_ERR_BAD_ARGUMENT, "%s: n_seq %d not in 1..1024", who, q.n_seq);
    if (q.layers < 1 || q.layers > 64 || q.layer < 0 || q.layer >= q.layers) FL_FAIL(FL_ERR_BAD_ARGUMENT, "%s: layer %d not below layers %d (1..64)", who, q.layer, q.layers);
    if (!q.count || !q.pos || !q.len || !q.seq_alloc || !q.v_transposed || !q.k_cache || !q.v_cache) FL_FAIL(FL_ERR_BAD_ARGUMENT, "%s: null per-sequence array", who);
    int64_t rows = 0;
    for (int s = 0; s < q.n_seq; s++) {
        if (!q.k_cache[s] || !q.v_cache[s]) FL_FAIL(FL_ERR_BAD_ARGUMENT, "%s: sequence %d: null cache", who, s);
        if (q.count[s] < 1 || q.pos[s] < 0 || q.len[s] < 0 || q.seq_alloc[s] < 1 || q.seq_alloc[s] > (1 << 24) || q.count[s] > (1 << 20))
            FL_FAIL(FL_ERR_BAD_ARGUMENT, "%s: sequence %d: count >= 1, pos >= 0, len >= 0, seq_alloc >= 1", who, s);
        if ((int64_t)q.len[s] + q.count[s] > q.seq_alloc[s])
            FL_FAIL(FL_ERR_BAD_ARGUMENT, "%s: sequence %d: len %d + count %d exceeds seq_alloc %d", who, s, q.len[s], q.count[s], q.seq_alloc[s]);
        if ((int64_t)q.pos[s] + q.count[s] > max_pos)
            FL_FAIL(FL_ERR_BAD_ARGUMENT, "%s: sequence %d: pos %d + count %d exceeds max_pos %lld", who, s, q.pos[s], q.count[s], (long long)max_pos);
        rows += q.count[s];
    }
    if (rows > (1 << 20)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "%s: too many rows", who);
    *rows_out = rows;
    return FL_OK;
}

// The sequences on the device: every cache an allocation of its own with a pristine copy beside it (a repeated launch starts from the
// caller's bytes), a StepState per sequence and the SeqRef array the batched and the packed kernels read.
struct RopeSeqsDev {
    std::vector<void *> k, v, k0, v0;
    std::vector<size_t> bytes;           // of one cache: layers * Hkv * seq_alloc * d elements
    std::vector<SeqRef> refs;
    StepState *st = nullptr;             // [n_seq]
    SeqRef *refs_dev = nullptr;
    size_t total = 0;                    // K and V bytes of all sequences

    int upload(OpScope &B, const fl_rope_seqs &q, int64_t Hkv, int64_t d, size_t es, const uint32_t *tokens) {
        const size_t n = (size_t)q.n_seq;
        k.resize(n); v.resize(n); k0.resize(n); v0.resize(n); bytes.resize(n); refs.assign(n, SeqRef{});
        std::vector<StepState> sts(n);
        FL_TRY(B.alloc(&st, sizeof(StepState) * n));
        for (size_t s = 0; s < n; s++) {
            bytes[s] = (size_t)q.layers * Hkv * q.seq_alloc[s] * d * es;
            total += 2 * bytes[s];
            FL_TRY(B.upload(&k0[s], q.k_cache[s], bytes[s])); FL_TRY(B.upload(&v0[s], q.v_cache[s], bytes[s]));
            FL_TRY(B.alloc(&k[s], bytes[s])); FL_TRY(B.alloc(&v[s], bytes[s]));
            sts[s] = StepState{};
            sts[s].token = tokens ? tokens[s] : 0u; sts[s].pos = (uint32_t)q.pos[s]; sts[s].len = (uint32_t)q.len[s]; sts[s].call0 = sts[s].len; sts[s].eos = -1;
            refs[s].st = st + s; refs[s].k = k[s]; refs[s].v = v[s]; refs[s].seq_alloc = q.seq_alloc[s]; refs[s].nsplit = 1;
        }
        FL_HIP(hipMemcpy(st, sts.data(), sizeof(StepState) * n, hipMemcpyHostToDevice));
        return B.upload(&refs_dev, refs.data(), sizeof(SeqRef) * n);
    }
    int restore(OpScope &B) {
        for (size_t s = 0; s < k.size(); s++) {
            FL_HIP(hipMemcpyAsync(k[s], k0[s], bytes[s], hipMemcpyDeviceToDevice, B.s));
            FL_HIP(hipMemcpyAsync(v[s], v0[s], bytes[s], hipMemcpyDeviceToDevice, B.s));
        }
        return FL_OK;
    }
    int download(unsigned char *o) const {                        // K | V of sequence 0, of sequence 1, ...
        for (size_t s = 0; s < k.size(); s++) {
            FL_HIP(hipMemcpy(o, k[s], bytes[s], hipMemcpyDeviceToHost)); o += bytes[s];
            FL_HIP(hipMemcpy(o, v[s], bytes[s], hipMemcpyDeviceToHost)); o += bytes[s];
        }
        return FL_OK;
    }
    void give_back(const fl_rope_seqs &q, const unsigned char *o) const {
        for (size_t s = 0; s < k.size(); s++) {
            memcpy(q.k_cache[s], o, bytes[s]); o += bytes[s];
            memcpy(q.v_cache[s], o, bytes[s]); o += bytes[s];
        }
    }
};

// `repeat` runs of run() from the caller's caches and a NaN-filled q: the bytes q | caches of the first one into `first`, FL_ERR_HIP if a
// later one differs
template <typename Run>
int rope_op_repeat(OpScope &B, const char *who, RopeSeqsDev &sq, void *qd, size_t qbytes, float *xo, size_t xbytes, int repeat, std::vector<unsigned char> &first, Run run) {
    std::vector<unsigned char> again;
    for (int rep = 0; rep < repeat; rep++) {
        FL_TRY(sq.restore(B));
        FL_HIP(hipMemsetAsync(qd, 0xff, qbytes, B.s));            // NaN pattern: an element no launch writes shows up
        if (xo) FL_HIP(hipMemsetAsync(xo, 0xff, xbytes, B.s));
        FL_TRY(run());
        FL_HIP(hipStreamSynchronize(B.s));
        std::vector<unsigned char> &o = rep ? again : first;
        o.resize(qbytes + xbytes + sq.total);
        FL_HIP(hipMemcpy(o.data(), qd, qbytes, hipMemcpyDeviceToHost));
        if (xo) FL_HIP(hipMemcpy(o.data() + qbytes, xo, xbytes, hipMemcpyDeviceToHost));
        FL_TRY(sq.download(o.data() + qbytes + xbytes));
        if (rep && first != again) FL_FAIL(FL_ERR_HIP, "%s: launch %d gave other bytes than the first", who, rep);
    }
    return FL_OK;
}

// the fl_op_rope_kv checks that need no device
int rope_kv_check(const fl_rope_kv_args *a, int64_t *rows_out) {
    if (!a) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_rope_kv: null args");
    if (a->struct_size != sizeof(fl_rope_kv_args)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_rope_kv: struct_size %zu, expected %zu", a->struct_size, sizeof(fl_rope_kv_args));
    if (a->form < 0 || a->form > 2) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_rope_kv: form %d not in 0..2", a->form);
    if (!a->qkv) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_rope_kv: null qkv");
    if (a->n_slab < 1 || a->n_slab > 64) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_rope_kv: n_slab %d not in 1..64", a->n_slab);
    if (a->repeat < 1 || a->repeat > 8) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_rope_kv: repeat %d not in 1..8", a->repeat);
    FL_TRY(rope_seqs_check("fl_op_rope_kv", a->seqs, a->dtype, a->H, a->Hkv, a->d, a->max_pos, a->cos_tab, a->sin_tab, a->q_out, rows_out));
    const fl_rope_seqs &q = a->seqs;
    if (a->form == 0 && q.n_seq != 1) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_rope_kv: form 0 takes one sequence");
    if (a->form == 1) {
        for (int s = 0; s < q.n_seq; s++) {
            if (q.count[s] != 1) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_rope_kv: form 1 takes one row per sequence");
            if ((q.v_transposed[s] != 0) != (q.v_transposed[0] != 0)) FL_FAIL(FL_ERR_UNSUPPORTED, "fl_op_rope_kv: form 1: one value layout for the whole batch");
        }
        if (a->dtype == FL_DTYPE_F32 && q.v_transposed[0]) FL_FAIL(FL_ERR_UNSUPPORTED, "fl_op_rope_kv: form 1: fp32 caches keep V row-major");
    }
    return FL_OK;
}

// the fl_op_qkv_rope checks that need no device
int qkv_rope_check(const fl_qkv_rope_args *a) {
    if (!a) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_qkv_rope: null args");
    if (a->struct_size != sizeof(fl_qkv_rope_args)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_qkv_rope: struct_size %zu, expected %zu", a->struct_size, sizeof(fl_qkv_rope_args));
    if (a->form < 0 || a->form > 3) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_qkv_rope: form %d not in 0..3", a->form);
    if (!a->w || !a->norm_w) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_qkv_rope: null argument (w, norm_w)");
    if (a->T <= 0 || a->T > (1 << 20) || a->K <= 0 || a->K % 8) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_qkv_rope: bad shape (K must be a multiple of 8)");
    if (a->repeat < 1 || a->repeat > 8) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_qkv_rope: repeat %d not in 1..8", a->repeat);
    if (a->n_slab < 0 || a->n_slab > 64 || (a->n_slab > 0) != (a->delta != nullptr)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_qkv_rope: n_slab 0..64, with delta exactly when it is not 0");
    if (a->embed) {
        if (a->x_res || a->delta || !a->tokens || a->vocab < 1) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_qkv_rope: embed takes tokens and a vocab size, and neither x_res nor delta");
        for (int64_t t = 0; t < a->T; t++)
            if ((int64_t)a->tokens[t] >= a->vocab) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_qkv_rope: tokens[%lld] = %u is not below vocab %lld", (long long)t, a->tokens[t], (long long)a->vocab);
    } else if (!a->x_res) {
        FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_qkv_rope: null x_res (and no embed)");
    }
    int64_t rows = 0;
    FL_TRY(rope_seqs_check("fl_op_qkv_rope", a->seqs, a->dtype, a->H, a->Hkv, a->d, a->max_pos, a->cos_tab, a->sin_tab, a->q_out, &rows));
    if (rows != a->T) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_qkv_rope: the sequences' counts give %lld rows, T is %lld", (long long)rows, (long long)a->T);
    const fl_rope_seqs &q = a->seqs;
    const int64_t N = (a->H + 2 * a->Hkv) * a->d;
    if (a->form != 3 && q.n_seq != 1) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_qkv_rope: form %d takes one sequence", a->form);
    if (a->form == 1) {
        if (a->T != 1) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_qkv_rope: form 1: the single-sequence stream takes one row");
        if (!gemv_norm_supported(a->dtype, N, a->K)) FL_FAIL(FL_ERR_UNSUPPORTED, "fl_op_qkv_rope: form 1: the norm prologue needs K <= 6144");
    } else if (a->form == 2) {
        if (a->T != 1) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_qkv_rope: form 2: the single-sequence stream takes one row");
        if (!a->w_scale) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_qkv_rope: form 2: null w_scale");
        if (a->dtype != FL_DTYPE_BF16 || a->n_slab > 1) FL_FAIL(FL_ERR_UNSUPPORTED, "fl_op_qkv_rope: form 2: bf16 activations, at most one delta vector");
        if (!gemv_w8_norm_supported(N, a->K)) FL_FAIL(FL_ERR_UNSUPPORTED, "fl_op_qkv_rope: form 2: K a multiple of 16, at most 6144");
    } else if (a->form == 3) {
        if (a->T > 8) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_qkv_rope: form 3: at most 8 rows");
        if (q.n_seq != a->T) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_qkv_rope: form 3: one sequence per row");
        if (a->dtype != FL_DTYPE_BF16) FL_FAIL(FL_ERR_UNSUPPORTED, "fl_op_qkv_rope: form 3: bf16");
        for (int s = 0; s < q.n_seq; s++)
            if (!q.v_transposed[s]) FL_FAIL(FL_ERR_UNSUPPORTED, "fl_op_qkv_rope: form 3: the batched stream appends to transposed value caches");
        if (gemv_batch_ksplit((int)a->T, a->K, 0, EPI_QKV_ROPE) != 1) FL_FAIL(FL_ERR_UNSUPPORTED, "fl_op_qkv_rope: form 3: K %lld needs K slices, which the RoPE epilogue cannot take", (long long)a->K);
    }
    return FL_OK;
}

// the fl_op_encoder_rows checks, none of which needs a device; *T_out: the rows of the call
int encoder_rows_check(const fl_encoder_rows_args *a, int64_t *T_out) {
    if (!a) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_encoder_rows: null args");
    if (a->struct_size != sizeof(fl_encoder_rows_args)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_encoder_rows: struct_size %zu, expected %zu", a->struct_size, sizeof(fl_encoder_rows_args));
    if (a->form < 0 || a->form > 3) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_encoder_rows: form %d not in 0..3", a->form);
    if (a->dtype != FL_DTYPE_BF16 && a->dtype != FL_DTYPE_F32) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_encoder_rows: dtype must be bf16 or f32");
    if (a->repeat < 1 || a->repeat > 8) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_encoder_rows: repeat %d not in 1..8", a->repeat);
    if (!a->out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_encoder_rows: null out");
    if (a->h < 1 || a->h > 65536) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_encoder_rows: h %lld not in 1..65536", (long long)a->h);
    if (a->form != 3 && a->h % 8) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_encoder_rows: form %d: the row width %lld must be a multiple of 8", a->form, (long long)a->h);
    if (a->form == 1 || a->form == 2) {
        if (a->n_slab < 1 || a->n_slab > 8) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_encoder_rows: n_slab %d not in 1..8", a->n_slab);
        if (a->T < 1 || a->T > (1 << 20)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_encoder_rows: T %lld not in 1..2^20", (long long)a->T);
        if (!a->slabs) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_encoder_rows: null slabs");
        *T_out = a->T;
    } else {
        int64_t longest = 0;
        if (a->form == 0 && (a->P < 1 || a->P > (1 << 20) || a->vocab < 1 || a->vocab > (1 << 24))) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_encoder_rows: P in 1..2^20, vocab in 1..2^24");
        if (a->n_seq > ((size_t)1 << 20)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_encoder_rows: n_seq above 2^20");
        FL_TRY(encoder_check_offsets(a->offsets, a->n_seq, a->form == 0 ? a->P : 0, 1 << 20, T_out, &longest));
    }
    if ((double)*T_out * (double)a->h * (a->form == 0 || a->form == 3 ? 1 : a->n_slab) > (double)(1 << 28)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_encoder_rows: more than 2^28 elements");
    if (a->form == 0) {
        if (!a->word || !a->pos || !a->ids) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_encoder_rows: form 0: null argument (word, pos, ids)");
        for (int64_t t = 0; t < *T_out; t++)
            if ((int64_t)a->ids[t] >= a->vocab) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_encoder_rows: ids[%lld] = %u is not below vocab %lld", (long long)t, a->ids[t], (long long)a->vocab);
    }
    if (a->form <= 1 && (!a->ln_w || !a->ln_b || !a->x_res_out)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_encoder_rows: form %d: null argument (ln_w, ln_b, x_res_out)", a->form);
    if ((a->form == 1 || a->form == 3) && !a->x) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_encoder_rows: form %d: null x", a->form);
    if (a->form == 2 && a->act != ENC_ACT_NONE && a->act != ENC_ACT_GELU_TANH && a->act != ENC_ACT_GELU_ERF)
        FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_encoder_rows: act %d (-1 none, 0 gelu_tanh, 1 gelu_erf)", a->act);
    return FL_OK;
}

// the fl_op_convert_slice checks, none of which needs a device: the slice inside the source, and every element's destination --
// found by walking the rows' and the columns' maps as convert_slice_kernel applies them -- inside dst
int convert_slice_check(const fl_convert_slice_args *a) {
    const int64_t kMax = (int64_t)1 << 26;
    if (!a) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_convert_slice: null args");
    if (a->struct_size != sizeof(fl_convert_slice_args)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_convert_slice: struct_size %zu, expected %zu", a->struct_size, sizeof(fl_convert_slice_args));
    if (!a->src || !a->dst) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_convert_slice: null argument (src, dst)");
    if (a->src_dtype < FL_DTYPE_F32 || a->src_dtype > FL_DTYPE_F16) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_convert_slice: src_dtype %d (f32, bf16 or f16)", a->src_dtype);
    if (a->dst_dtype != FL_DTYPE_F32 && a->dst_dtype != FL_DTYPE_BF16) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_convert_slice: dst_dtype %d (f32 or bf16)", a->dst_dtype);
    if (a->row_mode < 0 || a->row_mode > 2 || a->head_pad < 0 || a->head_pad > 2) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_convert_slice: row_mode and head_pad are 0, 1 or 2");
    if ((a->via_bf16 != 0 && a->via_bf16 != 1) || (a->via_bf16 && a->dst_dtype != FL_DTYPE_F32)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_convert_slice: via_bf16 is 0 or 1, and 1 only with an fp32 destination");
    if (a->R < 1 || a->C < 1 || a->R > kMax || a->C > kMax || a->R * a->C > kMax) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_convert_slice: source shape (1 .. 2^26 elements)");
    if (a->dst_rows < 1 || a->dst_ld < 1 || a->dst_rows > kMax || a->dst_ld > kMax || a->dst_rows * a->dst_ld > kMax)
        FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_convert_slice: destination shape (1 .. 2^26 elements)");
    if (a->r0 < 0 || a->c0 < 0 || a->rows < 1 || a->cols < 1 || a->rows > a->R - a->r0 || a->cols > a->C - a->c0)
        FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_convert_slice: the slice [%lld + %lld) x [%lld + %lld) leaves the source %lld x %lld", (long long)a->r0, (long long)a->rows,
                (long long)a->c0, (long long)a->cols, (long long)a->R, (long long)a->C);
    if (a->dst_row0 < 0 || a->dst_row0 >= a->dst_rows) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_convert_slice: dst_row0 %lld not in the destination's %lld rows", (long long)a->dst_row0, (long long)a->dst_rows);
    if (a->row_mode != 0 && (a->dst_row0 != 0 || a->head_pad == 1)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_convert_slice: the gate/up interleave takes neither a row offset nor padded head rows");
    if (a->head_pad != 0 && (a->dm < 2 || a->d < a->dm || a->dm % 2 || a->d % 2 || a->d > (1 << 20)))
        FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_convert_slice: head_pad needs 2 <= dm <= d <= 2^20, both even (dm %lld, d %lld)", (long long)a->dm, (long long)a->d);
    auto padded = [&](int64_t x) { const int64_t hd = x / a->dm, j = x % a->dm; return hd * a->d + (j < a->dm / 2 ? j : a->d / 2 + j - a->dm / 2); };
    for (int64_t r = 0; r < a->rows; r++) {
        const int64_t dr = a->head_pad == 1 ? a->dst_row0 + padded(r) : (a->row_mode == 0 ? a->dst_row0 + r : gateup_row(r, a->row_mode == 2));
        if (dr < 0 || dr >= a->dst_rows) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_convert_slice: source row %lld would land in row %lld of %lld", (long long)r, (long long)dr, (long long)a->dst_rows);
    }
    for (int64_t c = 0; c < a->cols; c++) {
        const int64_t dc = a->head_pad == 2 ? padded(c) : c;
        if (dc < 0 || dc >= a->dst_ld) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_convert_slice: source column %lld would land in column %lld of %lld", (long long)c, (long long)dc, (long long)a->dst_ld);
    }
    return FL_OK;
}

int attn_op_check_heads(int32_t dtype, int32_t layout, int64_t H, int64_t Hkv, int64_t d) {
    if ((dtype != FL_DTYPE_BF16 && dtype != FL_DTYPE_F32) || layout < 0 || layout > 1) FL_FAIL(FL_ERR_BAD_ARGUMENT, "dtype: bf16 or f32; layout: 0 plain, 1 MFMA");
    if (H < 1 || Hkv < 1 || H % Hkv != 0) FL_FAIL(FL_ERR_BAD_ARGUMENT, "bad head counts (H a multiple of Hkv)");
    if (d != 64 && d != 128) FL_FAIL(FL_ERR_UNSUPPORTED, "attention: head_dim %lld not supported (64 or 128)", (long long)d);
    if (layout == 1 && !attn_mfma_supported(dtype, H, Hkv, d)) FL_FAIL(FL_ERR_UNSUPPORTED, "MFMA attention: bf16, head_dim 64 / 128, at most 8 query heads per kv head");
    return FL_OK;
}

// the fl_op_attn_oproj_rep checks, none of which needs a device; *g: the launch's geometry and the two capacity rules
int attn_oproj_rep_check(const fl_attn_oproj_rep_args *a, AttnRepGeometry *g) {
    if (!a) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_attn_oproj_rep: null args");
    if (a->struct_size != sizeof(fl_attn_oproj_rep_args)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_attn_oproj_rep: struct_size %zu, expected %zu", a->struct_size, sizeof(fl_attn_oproj_rep_args));
    if (a->query_only != 0 && a->query_only != 1) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_attn_oproj_rep: query_only %d not 0 or 1", a->query_only);
    if (a->query_only ? !a->info_out : (!a->q || !a->k || !a->v || !a->w_o || !a->out)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_attn_oproj_rep: null argument");
    if (a->H < 1 || a->Hkv < 1 || a->H > 1024 || a->H % a->Hkv != 0) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_attn_oproj_rep: bad head counts (H %lld a multiple of Hkv %lld)", (long long)a->H, (long long)a->Hkv);
    if (a->d < 1 || a->d > 1024) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_attn_oproj_rep: head_dim %lld not in 1..1024", (long long)a->d);
    if (a->N < 1 || a->N > (1 << 20)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_attn_oproj_rep: N %lld not in 1..2^20", (long long)a->N);
    if (a->capacity < 1 || a->capacity > (1 << 20)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_attn_oproj_rep: capacity %lld not in 1..2^20", (long long)a->capacity);
    if (!a->query_only) {
        if (a->s_past < 0 || a->k_rows < a->s_past + 1 || a->capacity < a->k_rows) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_attn_oproj_rep: s_past + 1 <= k_rows <= capacity");
        if (!(a->pad_value == a->pad_value) || a->pad_value - a->pad_value != 0.f) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_attn_oproj_rep: pad_value must be finite");
        if (a->repeat < 1 || a->repeat > 16) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_attn_oproj_rep: repeat %d not in 1..16", a->repeat);
    }
    const int64_t sa = (a->capacity + 31) / 32 * 32;
    if (!attn_oproj_rep_geometry(a->H, a->Hkv, a->d, a->N, sa, g))
        FL_FAIL(FL_ERR_UNSUPPORTED, "fl_op_attn_oproj_rep: head shape not taken (head_dim 64 / 128, at most 8 query heads per kv head, 8 a multiple of Hkv, H * d <= 2048)");
    // The launch itself checks the head shape only -- in the model the capacity rule was applied when the cache was made -- and its
    // burst loop takes any number of tiles; the any-size rule's 32 tiles per slice is as far as this entry point goes.
    if (!a->query_only && !g->any_size) FL_FAIL(FL_ERR_UNSUPPORTED, "fl_op_attn_oproj_rep: a capacity of %lld rows is more than 32 key tiles per slice", (long long)sa);
    return FL_OK;
}

}  // namespace

extern "C" {

int fl_op_verify_select(const float *logits, int64_t T, int64_t V, const uint32_t *draft, uint32_t *argmax_out, int64_t *n_accepted_out) {
    return guarded([&]() -> int {
        if (!logits || !argmax_out || !n_accepted_out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument");
        if (T < 1 || T > kVerifyMaxRows || V <= 0 || V > (1 << 24)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "bad size (1 <= T <= %d)", kVerifyMaxRows);
        if (T > 1 && !draft) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null draft");
        OpScope B;
        FL_TRY(B.begin());
        float *lg; uint32_t *dr, *od;
        FL_TRY(B.upload(&lg, logits, (size_t)T * V * 4));
        FL_TRY(B.alloc(&dr, (size_t)kVerifyMaxRows * 4));
        FL_TRY(B.alloc(&od, (size_t)kVerifyWords * 4));
        if (T > 1) FL_HIP(hipMemcpy(dr, draft, (size_t)(T - 1) * 4, hipMemcpyHostToDevice));
        FL_HIP(hipMemset(od, 0, (size_t)kVerifyWords * 4));
        uint32_t host[2][kVerifyWords];
        for (int rep = 0; rep < 2; rep++) {                     // twice: the second launch meets the ticket word the first one put back
            FL_TRY(launch_verify_select(B.L, lg, V, (int)T, dr, od));
            FL_HIP(hipStreamSynchronize(B.s));
            FL_HIP(hipMemcpy(host[rep], od, sizeof host[rep], hipMemcpyDeviceToHost));
        }
        if (memcmp(host[0], host[1], sizeof host[0]) || host[1][kVerifyTicket] != 0)
            FL_FAIL(FL_ERR_HIP, "verify_select: a repeated launch gave another result (ticket %u)", host[1][kVerifyTicket]);
        for (int64_t t = 0; t < T; t++) argmax_out[t] = host[0][t];
        *n_accepted_out = (int64_t)host[0][kVerifyNacc];
        return FL_OK;
    });
}

int fl_op_verify_sample(const float *logits, int64_t T, int64_t V, const uint32_t *draft, const fl_sampler *sampler, uint32_t *tokens_out,
                        int64_t *n_accepted_out, int64_t *kept_out) {
    return guarded([&]() -> int {
        if (!logits || !sampler || !tokens_out || !n_accepted_out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument");
        if (T < 1 || T > kVerifyMaxRows || V <= 0 || V > (1 << 24)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "bad size (1 <= T <= %d)", kVerifyMaxRows);
        if (T > 1 && !draft) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null draft");
        SampleState ss;
        FL_TRY(make_sampler(sampler, V, &ss));
        if (!ss.on) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_verify_sample: temperature below 1e-7 is ArgMax (fl_op_verify_select)");
        OpScope B;
        FL_TRY(B.begin());
        float *lg, *sc; uint32_t *dr, *od, *kd;
        FL_TRY(B.upload(&lg, logits, (size_t)T * V * 4));
        FL_TRY(B.alloc(&sc, (size_t)T * V * 4));
        FL_TRY(B.alloc(&dr, (size_t)kVerifyMaxRows * 4));
        FL_TRY(B.alloc(&od, (size_t)kVerifyWords * 4));
        FL_TRY(B.alloc(&kd, (size_t)kVerifyMaxRows * 4));
        if (T > 1) FL_HIP(hipMemcpy(dr, draft, (size_t)(T - 1) * 4, hipMemcpyHostToDevice));
        FL_HIP(hipMemset(od, 0, (size_t)kVerifyWords * 4));
        uint32_t host[2][kVerifyWords], kept[2][kVerifyMaxRows];
        for (int rep = 0; rep < 2; rep++) {                     // twice: the second launch meets the ticket word the first one put back
            FL_HIP(hipMemsetAsync(kd, 0, (size_t)kVerifyMaxRows * 4, B.s));
            FL_TRY(launch_verify_sample(B.L, lg, V, (int)T, dr, ss, sc, od, kd));
            FL_HIP(hipStreamSynchronize(B.s));
            FL_HIP(hipMemcpy(host[rep], od, sizeof host[rep], hipMemcpyDeviceToHost));
            FL_HIP(hipMemcpy(kept[rep], kd, sizeof kept[rep], hipMemcpyDeviceToHost));
        }
        if (memcmp(host[0], host[1], sizeof host[0]) || memcmp(kept[0], kept[1], sizeof kept[0]) || host[1][kVerifyTicket] != 0)
            FL_FAIL(FL_ERR_HIP, "verify_sample: a repeated launch gave another result (ticket %u)", host[1][kVerifyTicket]);
        for (int64_t t = 0; t < T; t++) tokens_out[t] = host[0][t];
        if (kept_out) for (int64_t t = 0; t < T; t++) kept_out[t] = (int64_t)kept[0][t];
        *n_accepted_out = (int64_t)host[0][kVerifyNacc];
        return FL_OK;
    });
}

int fl_op_verify_sample_time(const float *logits, int64_t T, int64_t V, const fl_sampler *sampler, const int32_t *iters, double *ms_out) {
    return guarded([&]() -> int {
        if (!logits || !sampler || !iters || !ms_out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument");
        if (T < 1 || T > kVerifyMaxRows || V <= 0 || V > (1 << 24)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "bad size");
        for (int f = 0; f < 2; f++) if (iters[f] < 0 || iters[f] > (1 << 20)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "bad iteration count");
        SampleState ss;
        FL_TRY(make_sampler(sampler, V, &ss));
        if (!ss.on) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_verify_sample_time: temperature below 1e-7 is ArgMax");
        OpScope B;
        FL_TRY(B.begin());
        StepState st{}; st.eos = -1;
        float *lg, *sc; uint32_t *dr, *od; StepState *std_; SampleState *ssd;
        FL_TRY(B.upload(&lg, logits, (size_t)T * V * 4));
        FL_TRY(B.alloc(&sc, (size_t)T * V * 4));
        FL_TRY(B.alloc(&dr, (size_t)kVerifyMaxRows * 4));
        FL_TRY(B.alloc(&od, (size_t)kVerifyWords * 4));
        FL_TRY(B.upload(&std_, &st, sizeof st));
        FL_TRY(B.upload(&ssd, &ss, sizeof ss));
        FL_HIP(hipMemset(dr, 0, (size_t)kVerifyMaxRows * 4));
        FL_HIP(hipMemset(od, 0, (size_t)kVerifyWords * 4));
        FL_HIP(hipEventCreate(&B.e0)); FL_HIP(hipEventCreate(&B.e1));
        // form 0: the T rows in one launch; form 1: T one-row selection launches of the same rows (the step state does not advance)
        for (int form = 0; form < 2; form++) {
            ms_out[form] = 0.0;
            if (iters[form] == 0) continue;
            auto run = [&]() -> int {
                if (form == 0) return launch_verify_sample(B.L, lg, V, (int)T, dr, ss, sc, od, nullptr);
                for (int64_t t = 0; t < T; t++) FL_TRY(launch_select_advance(B.L, lg + (size_t)t * V, V, std_, ssd, sc + (size_t)t * V, od, 0));
                return FL_OK;
            };
            FL_TRY(run());                                      // warm
            FL_HIP(hipStreamSynchronize(B.s));
            FL_HIP(hipEventRecord(B.e0, B.s));
            for (int i = 0; i < iters[form]; i++) FL_TRY(run());
            FL_HIP(hipEventRecord(B.e1, B.s));
            FL_HIP(hipEventSynchronize(B.e1));
            float ms = 0.f; FL_HIP(hipEventElapsedTime(&ms, B.e0, B.e1));
            ms_out[form] = ms / iters[form];
        }
        return FL_OK;
    });
}

int fl_op_verify_packed(const float *logits, int64_t T, int64_t V, size_t n_seq, const size_t *offsets, const uint32_t *ids, const fl_sampler *samplers,
                        int64_t block_rows, uint32_t *tokens_out, int64_t *n_acc_out, int64_t *kept_out, int32_t iters, double *ms_out) {
    return guarded([&]() -> int {
        if (!logits || !offsets || !ids || !tokens_out || !n_acc_out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_verify_packed: null argument");
        if (T < 1 || T > kVerifyPackedMaxRows || V <= 0 || V > (1 << 24)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_verify_packed: bad size (1 <= T <= %d)", kVerifyPackedMaxRows);
        if (n_seq < 1 || n_seq > (size_t)kMaxBatch) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_verify_packed: n_seq %zu not in 1..%d", n_seq, kMaxBatch);
        if (block_rows < 0 || iters < 0 || iters > (1 << 20)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_verify_packed: negative block_rows or a bad iteration count");
        if (offsets[0] != 0 || offsets[n_seq] != (size_t)T) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_verify_packed: offsets must run from 0 to T");
        std::vector<PackedRow> rows;
        std::vector<int> off(n_seq), cnt(n_seq);
        std::vector<SampleState> ss(n_seq);
        bool any_sampled = false;
        for (size_t s = 0; s < n_seq; s++) {
            if (offsets[s + 1] <= offsets[s] || offsets[s + 1] - offsets[s] > (size_t)kVerifyMaxRows || offsets[s + 1] > (size_t)T)
                FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_verify_packed: member %zu must have 1..%d rows", s, kVerifyMaxRows);
            off[s] = (int)offsets[s]; cnt[s] = (int)(offsets[s + 1] - offsets[s]);
            for (int t = 0; t < cnt[s]; t++) rows.push_back(PackedRow{(int)s, t});
            FL_TRY(make_sampler(samplers ? samplers + s : nullptr, V, &ss[s]));
            any_sampled |= ss[s].on != 0;
        }
        for (int64_t r = 0; r < T; r++) if ((int64_t)ids[r] >= V) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_verify_packed: ids[%lld] = %u is not below V = %lld", (long long)r, ids[r], (long long)V);
        const int64_t R = block_rows == 0 ? T : std::min<int64_t>(block_rows, T);
        OpScope B;
        FL_TRY(B.begin());
        float *lg, *sc = nullptr; uint32_t *od, *kd;
        VerifyPackedArgs a;
        FL_TRY(B.upload(&lg, logits, (size_t)T * V * 4));
        if (any_sampled) FL_TRY(B.alloc(&sc, (size_t)R * V * 4));
        PackedRow *rd; int *ofd, *cnd; SampleState *ssd; uint32_t *idd;
        FL_TRY(B.upload(&rd, rows.data(), rows.size() * sizeof(PackedRow)));
        FL_TRY(B.upload(&ofd, off.data(), n_seq * 4));
        FL_TRY(B.upload(&cnd, cnt.data(), n_seq * 4));
        FL_TRY(B.upload(&ssd, ss.data(), n_seq * sizeof(SampleState)));
        FL_TRY(B.upload(&idd, ids, (size_t)T * 4));
        FL_TRY(B.alloc(&od, (size_t)kVerifyPackedWords * 4));
        FL_TRY(B.alloc(&kd, (size_t)T * 4));
        FL_HIP(hipMemset(od, 0, (size_t)kVerifyPackedWords * 4));
        a.rows = rd; a.seq_off = ofd; a.seq_cnt = cnd; a.ss = ssd; a.ids = idd; a.out = od; a.kept = kd;
        auto pass = [&]() -> int {
            for (int64_t r0 = 0; r0 < T; r0 += R) {
                const int64_t n = std::min<int64_t>(R, T - r0);
                FL_TRY(launch_verify_packed(B.L, lg + (size_t)r0 * V, V, (int)r0, (int)n, (int)T, a, sc, any_sampled));
            }
            return FL_OK;
        };
        std::vector<uint32_t> host[2], kept[2];
        for (int rep = 0; rep < 2; rep++) {                     // twice: the second pass meets the ticket words the first one put back
            host[rep].resize(kVerifyPackedWords); kept[rep].resize((size_t)T);
            FL_HIP(hipMemsetAsync(kd, 0, (size_t)T * 4, B.s));
            FL_TRY(pass());
            FL_HIP(hipStreamSynchronize(B.s));
            FL_HIP(hipMemcpy(host[rep].data(), od, (size_t)kVerifyPackedWords * 4, hipMemcpyDeviceToHost));
            FL_HIP(hipMemcpy(kept[rep].data(), kd, (size_t)T * 4, hipMemcpyDeviceToHost));
        }
        if (host[0] != host[1] || kept[0] != kept[1]) FL_FAIL(FL_ERR_HIP, "verify_packed: a repeated pass gave another result");
        for (size_t s = 0; s < n_seq; s++)
            if (host[1][kVerifyPackedTicket + s] != 0 || host[1][kVerifyPackedNacc + s] >= (uint32_t)cnt[s])
                FL_FAIL(FL_ERR_HIP, "verify_packed: member %zu ended with ticket %u, accepted count %u", s, host[1][kVerifyPackedTicket + s], host[1][kVerifyPackedNacc + s]);
        for (int64_t t = 0; t < T; t++) tokens_out[t] = host[0][t];
        if (kept_out) for (int64_t t = 0; t < T; t++) kept_out[t] = (int64_t)kept[0][t];
        for (size_t s = 0; s < n_seq; s++) n_acc_out[s] = (int64_t)host[0][kVerifyPackedNacc + s];
        if (iters > 0 && ms_out) {
            FL_TRY(pass());                                     // warm
            FL_HIP(hipStreamSynchronize(B.s));
            FL_HIP(hipEventCreate(&B.e0)); FL_HIP(hipEventCreate(&B.e1));
            FL_HIP(hipEventRecord(B.e0, B.s));
            for (int i = 0; i < iters; i++) FL_TRY(pass());
            FL_HIP(hipEventRecord(B.e1, B.s));
            FL_HIP(hipEventSynchronize(B.e1));
            float ms = 0.f; FL_HIP(hipEventElapsedTime(&ms, B.e0, B.e1));
            *ms_out = ms / iters;
        }
        return FL_OK;
    });
}

int fl_op_logprobs(const float *logits, int64_t T, int64_t V, const uint32_t *chosen, int32_t top_n, float *token_logprob,
                   uint32_t *top_ids, float *top_logprobs) {
    return guarded([&]() -> int {
        if (!logits || !chosen || !token_logprob) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_logprobs: null logits, chosen or token_logprob");
        if (T < 1 || T > 64) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_logprobs: T %lld not in 1..64", (long long)T);
        if (V < 1 || V > (1 << 24)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_logprobs: V %lld not in 1..2^24", (long long)V);
        if (top_n < 0 || top_n > FL_LOGPROBS_MAX_TOP || top_n > V)
            FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_logprobs: top_n %d not in 0..min(%d, V = %lld)", top_n, FL_LOGPROBS_MAX_TOP, (long long)V);
        if (top_n > 0 && (!top_ids || !top_logprobs)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_logprobs: null top_ids or top_logprobs with top_n %d", top_n);
        for (int64_t t = 0; t < T; t++)
            if ((int64_t)chosen[t] >= V) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_logprobs: chosen[%lld] = %u is not below V = %lld", (long long)t, chosen[t], (long long)V);
        OpScope B;
        FL_TRY(B.begin());
        float *lg; uint32_t *ch; LogprobRec *recs; LogprobCtl *ctl;
        FL_TRY(B.upload(&lg, logits, (size_t)T * V * 4));
        FL_TRY(B.upload(&ch, chosen, (size_t)T * 4));
        FL_TRY(B.alloc(&recs, (size_t)T * sizeof(LogprobRec)));
        FL_TRY(B.alloc(&ctl, sizeof(LogprobCtl)));
        FL_TRY(launch_set_logprob_ctl(B.L, ctl, recs, (uint32_t)T, top_n));
        LogprobSrc src;
        src.ctl = ctl; src.chosen = ch;
        std::vector<LogprobRec> host[2];
        for (int rep = 0; rep < 2; rep++) {                     // twice: the gather's order in LDS differs from launch to launch, the result must not
            host[rep].resize((size_t)T);
            FL_HIP(hipMemsetAsync(recs, 0, (size_t)T * sizeof(LogprobRec), B.s));
            FL_TRY(launch_token_logprobs(B.L, lg, V, (int)T, src, 0));
            FL_HIP(hipStreamSynchronize(B.s));
            FL_HIP(hipMemcpy(host[rep].data(), recs, (size_t)T * sizeof(LogprobRec), hipMemcpyDeviceToHost));
        }
        if (memcmp(host[0].data(), host[1].data(), (size_t)T * sizeof(LogprobRec))) FL_FAIL(FL_ERR_HIP, "token_logprobs: a repeated launch gave another result");
        for (int64_t t = 0; t < T; t++) {
            token_logprob[t] = host[0][(size_t)t].chosen;
            for (int j = 0; j < top_n; j++) {
                top_ids[t * top_n + j] = host[0][(size_t)t].ids[j];
                top_logprobs[t * top_n + j] = host[0][(size_t)t].lps[j];
            }
        }
        return FL_OK;
    });
}

// the argument checks of fl_op_score / fl_op_score_time
static int op_score_check(const char *who, const float *logits, int64_t T, int64_t V, const uint32_t *targets, int32_t top_n) {
    if (!logits || !targets) FL_FAIL(FL_ERR_BAD_ARGUMENT, "%s: null logits or targets", who);
    if (T < 1 || T > 1024) FL_FAIL(FL_ERR_BAD_ARGUMENT, "%s: T %lld not in 1..1024", who, (long long)T);
    if (V < 1 || V > (1 << 24)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "%s: V %lld not in 1..2^24", who, (long long)V);
    if (top_n < 0 || top_n > FL_LOGPROBS_MAX_TOP || top_n > V)
        FL_FAIL(FL_ERR_BAD_ARGUMENT, "%s: top_n %d not in 0..min(%d, V = %lld)", who, top_n, FL_LOGPROBS_MAX_TOP, (long long)V);
    for (int64_t t = 0; t < T; t++)
        if (targets[t] != FL_SCORE_NO_TARGET && (int64_t)targets[t] >= V)
            FL_FAIL(FL_ERR_BAD_ARGUMENT, "%s: targets[%lld] = %u is not below V = %lld", who, (long long)t, targets[t], (long long)V);
    return FL_OK;
}

int fl_op_score(const float *logits, int64_t T, int64_t V, const uint32_t *targets, int32_t top_n, float *target_logprob, uint32_t *target_rank,
                uint32_t *top_ids, float *top_logprobs) {
    return guarded([&]() -> int {
        FL_TRY(op_score_check("fl_op_score", logits, T, V, targets, top_n));
        if (!target_logprob) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_score: null target_logprob");
        if (top_n > 0 && (!top_ids || !top_logprobs)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_score: null top_ids or top_logprobs with top_n %d", top_n);
        OpScope B;
        FL_TRY(B.begin());
        float *lg; uint32_t *tg; ScoreRec *recs;
        FL_TRY(B.upload(&lg, logits, (size_t)T * V * 4));
        FL_TRY(B.upload(&tg, targets, (size_t)T * 4));
        FL_TRY(B.alloc(&recs, (size_t)T * sizeof(ScoreRec)));
        std::vector<ScoreRec> host[2];
        for (int rep = 0; rep < 2; rep++) {                     // twice: the gather's order in LDS differs from launch to launch, the result must not
            host[rep].resize((size_t)T);
            FL_HIP(hipMemsetAsync(recs, 0, (size_t)T * sizeof(ScoreRec), B.s));
            FL_TRY(launch_score_rows(B.L, lg, V, (int)T, tg, top_n, recs));
            FL_HIP(hipStreamSynchronize(B.s));
            FL_HIP(hipMemcpy(host[rep].data(), recs, (size_t)T * sizeof(ScoreRec), hipMemcpyDeviceToHost));
        }
        if (memcmp(host[0].data(), host[1].data(), (size_t)T * sizeof(ScoreRec))) FL_FAIL(FL_ERR_HIP, "score_rows: a repeated launch gave another result");
        for (int64_t t = 0; t < T; t++) {
            const ScoreRec &r = host[0][(size_t)t];
            target_logprob[t] = r.lp.chosen;
            if (target_rank) target_rank[t] = r.rank;
            for (int j = 0; j < top_n; j++) {
                top_ids[t * top_n + j] = r.lp.ids[j];
                top_logprobs[t * top_n + j] = r.lp.lps[j];
            }
        }
        return FL_OK;
    });
}

int fl_op_score_time(const float *logits, int64_t T, int64_t V, const uint32_t *targets, int32_t top_n, int32_t iters, double *ms_out) {
    return guarded([&]() -> int {
        FL_TRY(op_score_check("fl_op_score_time", logits, T, V, targets, top_n));
        if (!ms_out || iters < 1 || iters > (1 << 20)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_score_time: null ms_out or a bad iteration count");
        OpScope B;
        FL_TRY(B.begin());
        float *lg; uint32_t *tg; ScoreRec *recs;
        FL_TRY(B.upload(&lg, logits, (size_t)T * V * 4));
        FL_TRY(B.upload(&tg, targets, (size_t)T * 4));
        FL_TRY(B.alloc(&recs, (size_t)T * sizeof(ScoreRec)));
        FL_TRY(launch_score_rows(B.L, lg, V, (int)T, tg, top_n, recs));     // warm
        FL_HIP(hipStreamSynchronize(B.s));
        FL_HIP(hipEventCreate(&B.e0)); FL_HIP(hipEventCreate(&B.e1));
        FL_HIP(hipEventRecord(B.e0, B.s));
        for (int i = 0; i < iters; i++) FL_TRY(launch_score_rows(B.L, lg, V, (int)T, tg, top_n, recs));
        FL_HIP(hipEventRecord(B.e1, B.s));
        FL_HIP(hipEventSynchronize(B.e1));
        float ms = 0.f; FL_HIP(hipEventElapsedTime(&ms, B.e0, B.e1));
        *ms_out = ms / iters;
        return FL_OK;
    });
}

int fl_op_logit_rules(const float *logits, int64_t B, int64_t V, uint32_t *words, const float *biases, const float *scalars,
                      const uint32_t *tokens, int32_t count_input, const uint8_t *has_rules, float *out) {
    return guarded([&]() -> int {
        if (!logits || !words || !biases || !scalars || !tokens || !out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_logit_rules: null argument");
        if (B < 1 || B > 64) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_logit_rules: B %lld not in 1..64", (long long)B);
        if (V < 1 || V > (1 << 24)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_logit_rules: V %lld not in 1..2^24", (long long)V);
        OpScope S;
        FL_TRY(S.begin());
        // the rows back to back as a batch keeps them ([B][V]: with an odd V the rows b > 0 start off a 16-byte boundary); every
        // row's table an allocation of its own, as every cache's is
        float *lg, *od; uint32_t *tk; LogitRulesCtl *ctl; LogitRulesCtl **ctls;
        FL_TRY(S.upload(&lg, logits, (size_t)B * V * 4));
        FL_TRY(S.alloc(&od, (size_t)B * V * 4));
        FL_TRY(S.upload(&tk, tokens, (size_t)B * 4));
        FL_TRY(S.alloc(&ctl, (size_t)B * sizeof(LogitRulesCtl)));
        std::vector<LogitRuleEntry *> tabs((size_t)B);
        std::vector<LogitRulesCtl *> ptrs((size_t)B, nullptr);
        std::vector<LogitRuleEntry> img((size_t)V);
        for (int64_t b = 0; b < B; b++) {
            for (int64_t j = 0; j < V; j++) img[(size_t)j] = LogitRuleEntry{words[b * V + j], biases[b * V + j]};
            FL_TRY(S.upload(&tabs[(size_t)b], img.data(), (size_t)V * sizeof(LogitRuleEntry)));
            const LogitRulesCtl value{scalars[3 * b], scalars[3 * b + 1], scalars[3 * b + 2], count_input ? 1u : 0u, tabs[(size_t)b], nullptr};
            FL_TRY(launch_set_logit_rules_ctl(S.L, ctl + b, value));
            if (!has_rules || has_rules[b]) ptrs[(size_t)b] = ctl + b;
        }
        FL_TRY(S.upload(&ctls, ptrs.data(), (size_t)B * sizeof(LogitRulesCtl *)));
        LogitRulesSrc src;
        src.ctls = ctls; src.tokens = tk; src.out = od;
        FL_TRY(launch_logit_rules(S.L, lg, V, (int)B, src));
        FL_HIP(hipStreamSynchronize(S.s));
        FL_HIP(hipMemcpy(out, od, (size_t)B * V * 4, hipMemcpyDeviceToHost));
        for (int64_t b = 0; b < B; b++) {
            FL_HIP(hipMemcpy(img.data(), tabs[(size_t)b], (size_t)V * sizeof(LogitRuleEntry), hipMemcpyDeviceToHost));
            for (int64_t j = 0; j < V; j++) words[b * V + j] = img[(size_t)j].word;
        }
        return FL_OK;
    });
}

int fl_op_guide_mask(const float *logits, int64_t B, int64_t V, const fl_guide_desc *desc, const uint32_t *states, const uint32_t *tokens,
                     const uint8_t *has_guide, float *out, uint32_t *next_states) {
    return guarded([&]() -> int {
        if (!logits || !states || !tokens || !out || !next_states) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_guide_mask: null argument");
        if (B < 1 || B > 64) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_guide_mask: B %lld not in 1..64", (long long)B);
        if (V < 1 || V > (1 << 24)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_guide_mask: V %lld not in 1..2^24", (long long)V);
        FL_TRY(check_guide(desc, V));
        for (int64_t b = 0; b < B; b++)
            if (states[b] >= desc->n_states) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_guide_mask: states[%lld] = %u is not below n_states %u", (long long)b, states[b], desc->n_states);
        OpScope S;
        FL_TRY(S.begin());
        const size_t ns = desc->n_states, nnz = (size_t)desc->row_ptr[ns];
        float *lg, *od; uint32_t *tk, *ltok, *lnext; uint64_t *rp; GuideCtl *ctl; GuideCtl **ctls;
        FL_TRY(S.upload(&lg, logits, (size_t)B * V * 4));              // the rows back to back as a batch keeps them
        FL_TRY(S.alloc(&od, (size_t)B * V * 4));
        FL_TRY(S.upload(&tk, tokens, (size_t)B * 4));
        FL_TRY(S.upload(&rp, desc->row_ptr, (ns + 1) * 8));
        FL_TRY(S.upload(&ltok, desc->tokens, nnz * 4));
        FL_TRY(S.upload(&lnext, desc->next, nnz * 4));
        FL_TRY(S.alloc(&ctl, (size_t)B * sizeof(GuideCtl)));
        std::vector<GuideCtl *> ptrs((size_t)B, nullptr);
        for (int64_t b = 0; b < B; b++) if (!has_guide || has_guide[b]) ptrs[(size_t)b] = ctl + b;
        FL_TRY(S.upload(&ctls, ptrs.data(), (size_t)B * sizeof(GuideCtl *)));
        GuideSrc src;
        src.ctls = ctls; src.tokens = tk; src.out = od;
        std::vector<float> rows[2];
        std::vector<GuideCtl> back[2];
        for (int rep = 0; rep < 2; rep++) {                               // twice: workgroups search and fill in any order, the result must not depend on it
            rows[rep].resize((size_t)B * V);
            back[rep].resize((size_t)B);
            for (int64_t b = 0; b < B; b++)
                FL_TRY(launch_set_guide_ctl(S.L, ctl + b, GuideCtl{rp, ltok, lnext, nullptr, {states[b], states[b]}}));
            FL_HIP(hipMemsetAsync(od, 0x55, (size_t)B * V * 4, S.s));
            FL_TRY(launch_guide_mask(S.L, lg, V, (int)B, src));
            FL_HIP(hipStreamSynchronize(S.s));
            FL_HIP(hipMemcpy(rows[rep].data(), od, (size_t)B * V * 4, hipMemcpyDeviceToHost));
            FL_HIP(hipMemcpy(back[rep].data(), ctl, (size_t)B * sizeof(GuideCtl), hipMemcpyDeviceToHost));
        }
        if (memcmp(rows[0].data(), rows[1].data(), (size_t)B * V * 4)) FL_FAIL(FL_ERR_HIP, "guide_mask: a repeated launch gave another row");
        for (int64_t b = 0; b < B; b++) {
            if (back[0][(size_t)b].state[0] != back[1][(size_t)b].state[0]) FL_FAIL(FL_ERR_HIP, "guide_mask: a repeated launch gave another state");
            next_states[b] = back[0][(size_t)b].state[0];                 // (a row without a guide: the state the block was set to)
        }
        memcpy(out, rows[0].data(), (size_t)B * V * 4);
        return FL_OK;
    });
}

// fl_op_verify_adjust (out) and fl_op_verify_adjust_time (ms_out: `iters` launches between two events, nothing comes back)
static int op_verify_adjust(const float *logits, int64_t T, int64_t V, const uint32_t *ids, uint32_t *words, const float *biases, const float *scalars,
                            const fl_guide_desc *desc, const uint32_t *states, float *out, int32_t iters, double *ms_out) {
    return guarded([&]() -> int {
        if (!logits || !ids || (!out && !ms_out)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_verify_adjust: null argument");
        if (ms_out && (iters < 1 || iters > (1 << 20))) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_verify_adjust_time: a bad iteration count");
        if (T < 1 || T > kVerifyMaxRows) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_verify_adjust: T %lld not in 1..%d", (long long)T, kVerifyMaxRows);
        if (V < 1 || V > (1 << 24)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_verify_adjust: V %lld not in 1..2^24", (long long)V);
        if (!words && !desc) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_verify_adjust: neither rules (words) nor a guide (desc)");
        if (words && (!biases || !scalars)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_verify_adjust: rules need words, biases and scalars");
        if (desc) {
            FL_TRY(check_guide(desc, V));
            if (!states) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_verify_adjust: a guide needs states");
            for (int64_t t = 0; t < T; t++)
                if (states[t] >= desc->n_states) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_verify_adjust: states[%lld] = %u is not below n_states %u", (long long)t, states[t], desc->n_states);
        }
        OpScope S;
        FL_TRY(S.begin());
        // the rows back to back as a verify step keeps them ([T][V]: with an odd V the rows i > 0 start off a 16-byte boundary)
        float *lg, *od; LogitRuleEntry *tab = nullptr; uint32_t *ltok = nullptr; uint64_t *rp = nullptr;
        FL_TRY(S.upload(&lg, logits, (size_t)T * V * 4));
        FL_TRY(S.alloc(&od, (size_t)T * V * 4));
        std::vector<LogitRuleEntry> img;
        if (words) {
            img.resize((size_t)V);
            for (int64_t j = 0; j < V; j++) img[(size_t)j] = LogitRuleEntry{words[j], biases[j]};
            FL_TRY(S.upload(&tab, img.data(), (size_t)V * sizeof(LogitRuleEntry)));
        }
        if (desc) {
            const size_t ns = desc->n_states, nnz = (size_t)desc->row_ptr[ns];
            FL_TRY(S.upload(&rp, desc->row_ptr, (ns + 1) * 8));
            FL_TRY(S.upload(&ltok, desc->tokens, nnz * 4));
        }
        VerifyAdjustArgs a;
        for (int64_t t = 0; t < T; t++) { a.ids[t] = ids[t]; a.states[t] = desc ? states[t] : 0u; }
        a.table = tab;
        if (words) { a.rp = scalars[0]; a.fp = scalars[1]; a.pp = scalars[2]; }
        a.row_ptr = rp; a.tokens = ltok; a.out = od;
        if (ms_out) {
            FL_TRY(launch_verify_adjust(S.L, lg, V, (int)T, a));          // warm
            FL_HIP(hipStreamSynchronize(S.s));
            FL_HIP(hipEventCreate(&S.e0)); FL_HIP(hipEventCreate(&S.e1));
            FL_HIP(hipEventRecord(S.e0, S.s));
            for (int i = 0; i < iters; i++) FL_TRY(launch_verify_adjust(S.L, lg, V, (int)T, a));
            FL_HIP(hipEventRecord(S.e1, S.s));
            FL_HIP(hipEventSynchronize(S.e1));
            float ms = 0.f; FL_HIP(hipEventElapsedTime(&ms, S.e0, S.e1));
            *ms_out = ms / iters;
            return FL_OK;
        }
        std::vector<float> rows[2];
        for (int rep = 0; rep < 2; rep++) {                               // twice: workgroups count, search and fill in any order, the result must not depend on it
            rows[rep].resize((size_t)T * V);
            FL_HIP(hipMemsetAsync(od, 0x55, (size_t)T * V * 4, S.s));
            FL_TRY(launch_verify_adjust(S.L, lg, V, (int)T, a));
            FL_HIP(hipStreamSynchronize(S.s));
            FL_HIP(hipMemcpy(rows[rep].data(), od, (size_t)T * V * 4, hipMemcpyDeviceToHost));
        }
        if (memcmp(rows[0].data(), rows[1].data(), (size_t)T * V * 4)) FL_FAIL(FL_ERR_HIP, "verify_adjust: a repeated launch gave another row");
        memcpy(out, rows[0].data(), (size_t)T * V * 4);
        if (words) {                                                      // the table as the launches left it: unchanged, if the kernel keeps its word
            FL_HIP(hipMemcpy(img.data(), tab, (size_t)V * sizeof(LogitRuleEntry), hipMemcpyDeviceToHost));
            for (int64_t j = 0; j < V; j++) words[j] = img[(size_t)j].word;
        }
        return FL_OK;
    });
}

int fl_op_verify_adjust(const float *logits, int64_t T, int64_t V, const uint32_t *ids, uint32_t *words, const float *biases, const float *scalars,
                        const fl_guide_desc *desc, const uint32_t *states, float *out) {
    if (!out) return guarded([&]() -> int { FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_verify_adjust: null out"); });
    return op_verify_adjust(logits, T, V, ids, words, biases, scalars, desc, states, out, 0, nullptr);
}

int fl_op_verify_adjust_time(const float *logits, int64_t T, int64_t V, const uint32_t *ids, const uint32_t *words, const float *biases,
                             const float *scalars, const fl_guide_desc *desc, const uint32_t *states, int32_t iters, double *ms_out) {
    if (!ms_out) return guarded([&]() -> int { FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_verify_adjust_time: null ms_out"); });
    return op_verify_adjust(logits, T, V, ids, const_cast<uint32_t *>(words), biases, scalars, desc, states, nullptr, iters, ms_out);
}

int fl_op_rules_count(uint32_t *words, int64_t V, const uint32_t *ids, int64_t n) {
    return guarded([&]() -> int {
        if (!words || (n > 0 && !ids)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_rules_count: null argument");
        if (n < 0 || n > kVerifyMaxRows) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_rules_count: n %lld not in 0..%d", (long long)n, kVerifyMaxRows);
        if (V < 1 || V > (1 << 24)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_rules_count: V %lld not in 1..2^24", (long long)V);
        OpScope S;
        FL_TRY(S.begin());
        std::vector<LogitRuleEntry> img((size_t)V);
        for (int64_t j = 0; j < V; j++) img[(size_t)j] = LogitRuleEntry{words[j], 0.f};
        LogitRuleEntry *tab;
        FL_TRY(S.upload(&tab, img.data(), (size_t)V * sizeof(LogitRuleEntry)));
        RulesCountArgs a;
        a.n = (int)n;
        for (int64_t r = 0; r < n; r++) a.ids[r] = ids[r];
        FL_TRY(launch_rules_count(S.L, tab, V, a));
        FL_HIP(hipStreamSynchronize(S.s));
        FL_HIP(hipMemcpy(img.data(), tab, (size_t)V * sizeof(LogitRuleEntry), hipMemcpyDeviceToHost));
        for (int64_t j = 0; j < V; j++) words[j] = img[(size_t)j].word;
        return FL_OK;
    });
}

int fl_op_encoder_attention(const void *q, const void *k, const void *v, const size_t *offsets, size_t n_seq, int64_t H, int64_t d,
                            int32_t dtype, float *out) {
    return guarded([&]() -> int {
        if (!q || !k || !v || !out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument");
        if (dtype != FL_DTYPE_BF16 && dtype != FL_DTYPE_F32) FL_FAIL(FL_ERR_BAD_ARGUMENT, "dtype must be bf16 or f32");
        if (H < 1 || H > 65535) FL_FAIL(FL_ERR_BAD_ARGUMENT, "bad head count");
        if (!encoder_attention_supported(d)) FL_FAIL(FL_ERR_UNSUPPORTED, "encoder attention: head_dim 32 or 64");
        int64_t T = 0, longest = 0;
        FL_TRY(encoder_check_offsets(offsets, n_seq, 1 << 18, 1 << 20, &T, &longest));
        OpScope B;
        FL_TRY(B.begin());
        const size_t es = dtype == FL_DTYPE_BF16 ? 2 : 4, n = (size_t)T * H * d;
        std::vector<int32_t> off(n_seq + 1);
        for (size_t s = 0; s <= n_seq; s++) off[s] = (int32_t)offsets[s];
        void *qd, *kd, *vd, *od; int32_t *offd;
        FL_TRY(B.upload(&qd, q, n * es)); FL_TRY(B.upload(&kd, k, n * es)); FL_TRY(B.upload(&vd, v, n * es));
        FL_TRY(B.upload(&offd, off.data(), (n_seq + 1) * 4));
        FL_TRY(B.alloc(&od, n * es));
        FL_HIP(hipMemset(od, 0xff, n * es));                       // NaN pattern: an element the kernel does not write shows up
        FL_TRY(launch_encoder_attention(B.L, dtype, qd, kd, vd, H * d, offd, (int64_t)n_seq, longest, T, H, d, 1.0f / sqrtf((float)d), od));
        FL_HIP(hipStreamSynchronize(B.s));
        return op_download(out, od, n, dtype);
    });
}

int fl_op_encoder_rows(const fl_encoder_rows_args *args) {
    return guarded([&]() -> int {
        int64_t T = 0;
        FL_TRY(encoder_rows_check(args, &T));
        const fl_encoder_rows_args &a = *args;
        OpScope B;
        FL_TRY(B.begin());
        const int form = a.form, dtype = a.dtype;
        const int64_t h = a.h;
        const size_t es = dtype == FL_DTYPE_BF16 ? 2 : 4, n = (size_t)T * h;
        const size_t xbytes = form <= 1 ? n * 4 : 0;                          // x_res_out
        const size_t obytes = form == 3 ? a.n_seq * (size_t)h * 4 : n * es;   // out
        void *word = nullptr, *pos = nullptr, *tt0 = nullptr, *od; uint32_t *ids = nullptr; int32_t *row_seq = nullptr, *offd = nullptr;
        float *x0 = nullptr, *xr = nullptr, *slabs = nullptr, *bias = nullptr, *lnw = nullptr, *lnb = nullptr;
        if (form == 0 || form == 3) {
            std::vector<int32_t> rs((size_t)T), off(a.n_seq + 1);
            for (size_t s = 0; s <= a.n_seq; s++) off[s] = (int32_t)a.offsets[s];
            for (size_t s = 0; s < a.n_seq; s++)
                for (size_t r = a.offsets[s]; r < a.offsets[s + 1]; r++) rs[r] = (int32_t)s;
            FL_TRY(B.upload(&offd, off.data(), (a.n_seq + 1) * 4));
            if (form == 0) FL_TRY(B.upload(&row_seq, rs.data(), (size_t)T * 4));
        }
        if (form == 0) {
            FL_TRY(B.upload(&word, a.word, (size_t)a.vocab * h * es)); FL_TRY(B.upload(&pos, a.pos, (size_t)a.P * h * es));
            if (a.tt0) FL_TRY(B.upload(&tt0, a.tt0, (size_t)h * es));
            FL_TRY(B.upload(&ids, a.ids, (size_t)T * 4));
        }
        if (form == 1 || form == 3) FL_TRY(B.upload(&x0, a.x, n * 4));
        if (form == 1 || form == 2) {
            FL_TRY(B.upload(&slabs, a.slabs, (size_t)a.n_slab * n * 4));
            if (a.bias) FL_TRY(B.upload(&bias, a.bias, (size_t)h * 4));
        }
        if (form <= 1) {
            FL_TRY(B.upload(&lnw, a.ln_w, (size_t)h * 4)); FL_TRY(B.upload(&lnb, a.ln_b, (size_t)h * 4));
            FL_TRY(B.alloc(&xr, xbytes));
        }
        FL_TRY(B.alloc(&od, obytes));
        std::vector<unsigned char> first, again;
        for (int rep = 0; rep < a.repeat; rep++) {
            // NaN pattern: an element no launch writes shows up.  Form 1 updates the residual stream in place: from the caller's rows each time.
            if (form == 0) FL_HIP(hipMemsetAsync(xr, 0xff, xbytes, B.s));
            if (form == 1) FL_HIP(hipMemcpyAsync(xr, x0, xbytes, hipMemcpyDeviceToDevice, B.s));
            FL_HIP(hipMemsetAsync(od, 0xff, obytes, B.s));
            if (form == 0) FL_TRY(launch_encoder_embed_ln(B.L, dtype, word, pos, tt0, ids, row_seq, offd, lnw, lnb, a.eps, xr, od, T, h));
            else if (form == 1) FL_TRY(launch_encoder_add_ln(B.L, dtype, xr, slabs, a.n_slab, (int64_t)n, bias, lnw, lnb, a.eps, od, T, h));
            else if (form == 2) FL_TRY(launch_encoder_bias_act(B.L, dtype, slabs, a.n_slab, (int64_t)n, bias, a.act, od, T, h));
            else FL_TRY(launch_encoder_pool_l2(B.L, x0, offd, (int64_t)a.n_seq, h, (float *)od));
            FL_HIP(hipStreamSynchronize(B.s));
            std::vector<unsigned char> &o = rep ? again : first;
            o.resize(xbytes + obytes);
            if (xbytes) FL_HIP(hipMemcpy(o.data(), xr, xbytes, hipMemcpyDeviceToHost));
            FL_HIP(hipMemcpy(o.data() + xbytes, od, obytes, hipMemcpyDeviceToHost));
            if (rep && first != again) FL_FAIL(FL_ERR_HIP, "fl_op_encoder_rows: launch %d gave other bytes than the first", rep);
        }
        if (xbytes) memcpy(a.x_res_out, first.data(), xbytes);
        memcpy(a.out, first.data() + xbytes, obytes);
        return FL_OK;
    });
}

int fl_op_sample_ex(const float *logits, int64_t V, const fl_sampler *sampler, int64_t n_draws, uint32_t *tokens_out, int64_t *kept_out) {
    return guarded([&]() -> int {
        if (!logits || !sampler || !tokens_out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument");
        if (V <= 0 || V > (1 << 24) || n_draws <= 0 || n_draws > (1 << 20)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "bad size");
        SampleState ss;
        FL_TRY(make_sampler(sampler, V, &ss));
        OpScope B;
        FL_TRY(B.begin());
        const bool kept_dev = kept_out && ss.filter;       // (no filter: every token is kept)
        StepState st{}; st.eos = -1;
        float *lg, *sc; StepState *std_; SampleState *ssd; uint32_t *od, *kept = nullptr;
        FL_TRY(B.upload(&lg, logits, (size_t)V * 4));
        FL_TRY(B.alloc(&sc, (size_t)V * 4));
        FL_TRY(B.upload(&std_, &st, sizeof st));
        FL_TRY(B.upload(&ssd, &ss, sizeof ss));
        FL_TRY(B.alloc(&od, (size_t)n_draws * 4));
        if (kept_dev) FL_TRY(B.alloc(&kept, (size_t)n_draws * 4));
        for (int64_t i = 0; i < n_draws; i++) {
            FL_TRY(launch_select_advance(B.L, lg, V, std_, ssd, sc, od, 1));
            if (kept_dev) FL_HIP(hipMemcpyAsync(kept + i, &ssd->kept, 4, hipMemcpyDeviceToDevice, B.s));
        }
        FL_HIP(hipStreamSynchronize(B.s));
        FL_HIP(hipMemcpy(tokens_out, od, (size_t)n_draws * 4, hipMemcpyDeviceToHost));
        if (kept_out) {
            std::vector<uint32_t> k((size_t)n_draws, (uint32_t)V);
            if (kept_dev) FL_HIP(hipMemcpy(k.data(), kept, (size_t)n_draws * 4, hipMemcpyDeviceToHost));
            for (int64_t i = 0; i < n_draws; i++) kept_out[i] = (int64_t)k[(size_t)i];
        }
        return FL_OK;
    });
}

int fl_op_sample(const float *logits, int64_t V, const fl_sampling *sampling, int64_t n_draws, uint32_t *tokens_out) {
    if (!sampling) return fl_op_sample_ex(logits, V, nullptr, n_draws, tokens_out, nullptr);
    const fl_sampler s = widen(*sampling);
    return fl_op_sample_ex(logits, V, &s, n_draws, tokens_out, nullptr);
}

int fl_op_linear(const void *x, const void *w, const float *bias, int64_t T, int64_t N, int64_t K, int32_t dtype,
                 int32_t epilogue, float *y, int32_t iters, double *ms_out) {
    return guarded([&]() -> int {
        if (!x || !w || !y) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument");
        if (dtype != FL_DTYPE_BF16 && dtype != FL_DTYPE_F32) FL_FAIL(FL_ERR_UNSUPPORTED, "dtype must be bf16 or f32");
        if (T <= 0 || N <= 0 || K <= 0 || K % 8) FL_FAIL(FL_ERR_BAD_ARGUMENT, "bad shape (K must be a multiple of 8)");
        if (epilogue == EPI_GATEUP && (N % 2)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "gate/up needs an even row count");
        OpScope B;
        FL_TRY(B.begin());
        const size_t es = dtype == FL_DTYPE_BF16 ? 2 : 4;
        const int64_t I = N / 2, Ip = (I + 15) / 16 * 16;
        const int64_t Nw = epilogue == EPI_GATEUP ? 2 * Ip : N;          // rows of the device matrix
        const int64_t Ny = epilogue == EPI_GATEUP ? Ip : N;              // columns of the device output
        const size_t wbytes = (size_t)Nw * K * es, ybytes = (size_t)T * Ny * (epilogue == EPI_GATEUP ? es : 4);
        const int op_split = tune(TK_OP_MAXSPLIT);
        const int max_split = (epilogue == EPI_F32 && !bias) ? (op_split > 0 ? op_split : std::max(4, ksplit_cap(T))) : 1;      // exercise split-K where the model would
        int nsplit = 1;
        void *xd, *wd, *yd; float *bd = nullptr;
        FL_TRY(B.upload(&xd, x, (size_t)T * K * es));
        FL_TRY(B.alloc(&wd, wbytes));
        FL_TRY(B.alloc(&yd, ybytes * max_split));
        if (epilogue == EPI_GATEUP) {
            void *ws;
            FL_TRY(B.upload(&ws, w, (size_t)N * K * es));
            FL_HIP(hipMemsetAsync(wd, 0, wbytes, B.s));
            FL_TRY(launch_convert_slice(B.L, dtype, ws, K, 0, 0, I, K, dtype, wd, K, 0, 1));
            FL_TRY(launch_convert_slice(B.L, dtype, ws, K, I, 0, I, K, dtype, wd, K, 0, 2));
        } else {
            FL_HIP(hipMemcpy(wd, w, (size_t)N * K * es, hipMemcpyHostToDevice));
            if (bias) FL_TRY(B.upload(&bd, bias, (size_t)N * 4));
        }
        // FL_OP_LINEAR_DMA=1: T <= 8 rows go through the batched-decode projection kernel (k_gemv_dma.hip) instead, so that
        // its weight-streaming rate can be measured (and its arithmetic tested) without a model around it
        const bool use_dma = tune(TK_OP_LINEAR_DMA) == 1;
        const bool dma = use_dma && dtype == FL_DTYPE_BF16 && T <= 32 && !bd && gemv_dma_supported((int)T, Nw, K, epilogue, 0) &&
                         gemv_dma_ksplit(K, Nw, epilogue) <= max_split;
        std::vector<const void *> W{wd};                                 // the copies of the device matrix a timed run rotates over
        auto make = [&](int) -> int {
            void *p;
            FL_TRY(B.alloc(&p, wbytes));
            FL_HIP(hipMemcpyAsync(p, wd, wbytes, hipMemcpyDeviceToDevice, B.s));
            W.push_back(p);
            return FL_OK;
        };
        auto run = [&](int c) -> int {
            if (!dma) return launch_linear(B.L, dtype, W[(size_t)c], xd, bd, yd, T, Nw, K, epilogue, nullptr, max_split, &nsplit);
            GemvBatchArgs ga;
            ga.W = W[(size_t)c]; ga.x = xd; ga.out = yd; ga.N = (int)Nw; ga.K = (int)K; ga.epi = epilogue; ga.pro = PRO_X; ga.B = (int)T;
            ga.nks = epilogue == EPI_F32 ? gemv_dma_ksplit(K, Nw, epilogue) : 1;
            nsplit = ga.nks;
            return launch_gemv_dma(B.L, ga);
        };
        FL_TRY(op_run(B, wbytes, iters, ms_out, make, run));
        if (epilogue == EPI_GATEUP) return op_download(y, yd, (size_t)T, (size_t)I, (size_t)Ip, dtype);      // without the padding columns
        FL_HIP(hipMemcpy(y, yd, ybytes, hipMemcpyDeviceToHost));
        if (nsplit > 1) {                                   // sum the split-K slabs in slab order, like rmsnorm_add does
            std::unique_ptr<float[]> tmp(new float[(size_t)T * Ny]);
            for (int sl = 1; sl < nsplit; sl++) {
                FL_HIP(hipMemcpy(tmp.get(), (char *)yd + (size_t)sl * ybytes, ybytes, hipMemcpyDeviceToHost));
                for (size_t i = 0; i < (size_t)T * Ny; i++) y[i] += tmp[i];
            }
        }
        return FL_OK;
    });
}

int fl_op_quantize_rows(const void *w, int32_t dtype, int64_t N, int64_t K, uint8_t *q_out, float *s_out) {
    return guarded([&]() -> int {
        if (!w || !q_out || !s_out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument");
        if (dtype != FL_DTYPE_BF16 && dtype != FL_DTYPE_F32) FL_FAIL(FL_ERR_UNSUPPORTED, "dtype must be bf16 or f32");
        if (N <= 0 || K <= 0 || K % 4 || N > (1 << 24)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "bad shape (K must be a multiple of 4)");
        OpScope B;
        FL_TRY(B.begin());
        const size_t es = dtype == FL_DTYPE_BF16 ? 2 : 4;
        void *wd; uint8_t *qd; float *sd;
        FL_TRY(B.upload(&wd, w, (size_t)N * K * es));
        FL_TRY(B.alloc(&qd, (size_t)N * K));
        FL_TRY(B.alloc(&sd, (size_t)N * 4));
        FL_TRY(launch_quantize_rows(B.L, dtype, wd, N, K, qd, sd, nullptr));
        FL_HIP(hipStreamSynchronize(B.s));
        FL_HIP(hipMemcpy(q_out, qd, (size_t)N * K, hipMemcpyDeviceToHost));
        FL_HIP(hipMemcpy(s_out, sd, (size_t)N * 4, hipMemcpyDeviceToHost));
        return FL_OK;
    });
}

int fl_op_gemv_w8(const void *x, const uint8_t *q, const float *s, const float *bias, int64_t N, int64_t K, int32_t epilogue,
                  float *y, int32_t iters, double *ms_out) {
    return guarded([&]() -> int {
        if (!x || !q || !s || !y) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument");
        if (N <= 0 || K <= 0 || N > (1 << 24)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "bad shape");
        if (epilogue != EPI_F32 && epilogue != EPI_GATEUP) FL_FAIL(FL_ERR_BAD_ARGUMENT, "epilogue must be 0 or 1");
        if (epilogue == EPI_GATEUP && ((N % 2) || bias)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "gate/up needs an even row count and takes no bias");
        if (!gemv_w8_supported(N, K)) FL_FAIL(FL_ERR_UNSUPPORTED, "K must be a multiple of 16 (a lane of the FP8 stream loads 16 weights), at most 81792");
        OpScope B;
        FL_TRY(B.begin());
        const int64_t I = N / 2, Ip = (I + 15) / 16 * 16;
        const int64_t Nw = epilogue == EPI_GATEUP ? 2 * Ip : N;          // rows of the device matrix
        const int64_t Ny = epilogue == EPI_GATEUP ? Ip : N;
        const size_t wbytes = (size_t)Nw * K, ybytes = (size_t)Ny * (epilogue == EPI_GATEUP ? 2 : 4);
        void *xd, *yd; uint8_t *qd; float *sd, *bd = nullptr;
        FL_TRY(B.upload(&xd, x, (size_t)K * 2));
        FL_TRY(B.alloc(&qd, wbytes));
        FL_TRY(B.alloc(&sd, (size_t)Nw * 4));
        FL_TRY(B.alloc(&yd, ybytes));
        if (epilogue == EPI_GATEUP) {
            uint8_t *qs; float *ss;
            FL_TRY(B.upload(&qs, q, (size_t)N * K));
            FL_TRY(B.upload(&ss, s, (size_t)N * 4));
            FL_HIP(hipMemsetAsync(qd, 0, wbytes, B.s));
            FL_HIP(hipMemsetAsync(sd, 0, (size_t)Nw * 4, B.s));
            FL_TRY(launch_w8_gateup_layout(B.L, qs, ss, I, K, qd, sd));
        } else {
            FL_HIP(hipMemcpy(qd, q, (size_t)N * K, hipMemcpyHostToDevice));
            FL_HIP(hipMemcpy(sd, s, (size_t)N * 4, hipMemcpyHostToDevice));
            if (bias) FL_TRY(B.upload(&bd, bias, (size_t)N * 4));
        }
        std::vector<const uint8_t *> Q{qd};                              // the copies of q a timed run rotates over
        auto make = [&](int) -> int {
            uint8_t *p;
            FL_TRY(B.alloc(&p, wbytes));
            FL_HIP(hipMemcpyAsync(p, qd, wbytes, hipMemcpyDeviceToDevice, B.s));
            Q.push_back(p);
            return FL_OK;
        };
        auto run = [&](int c) -> int {
            GemvArgs a;
            a.W = Q[(size_t)c]; a.x = xd; a.bias = bd; a.out = yd; a.N = (int)Nw; a.K = (int)K; a.epi = epilogue; a.pro = PRO_X;
            return launch_gemv_w8(B.L, a, sd);
        };
        FL_TRY(op_run(B, wbytes, iters, ms_out, make, run));
        if (epilogue == EPI_GATEUP) return op_download(y, yd, (size_t)I, FL_DTYPE_BF16);                    // without the padding columns
        FL_HIP(hipMemcpy(y, yd, ybytes, hipMemcpyDeviceToHost));
        return FL_OK;
    });
}

int fl_op_kv_copy(const void *src, void *dst, int64_t rows, int64_t width_bytes, int64_t src_pitch, int64_t dst_pitch, int32_t iters,
                  double *ms_out) {
    return guarded([&]() -> int {
        if (!src || !dst) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument");
        if (rows < 1 || width_bytes < 2 || rows > (int64_t)1 << 31) FL_FAIL(FL_ERR_BAD_ARGUMENT, "bad shape (rows >= 1, width_bytes >= 2)");
        KvCopyJob shape;                                     // width / pitch rules: the launch's own
        shape.rows = rows; shape.width = width_bytes; shape.spitch = src_pitch; shape.dpitch = dst_pitch;
        FL_TRY(kv_copy_check(shape));
        OpScope B;
        FL_TRY(B.begin());
        const size_t sbytes = (size_t)rows * (size_t)src_pitch, dbytes = (size_t)rows * (size_t)dst_pitch;
        std::vector<void *> sd, dd;                          // the buffer pairs a timed run rotates over
        auto make = [&](int) -> int {
            void *p;
            FL_TRY(B.upload(&p, src, sbytes)); sd.push_back(p);
            FL_TRY(B.upload(&p, dst, dbytes)); dd.push_back(p);
            return FL_OK;
        };
        auto run = [&](int c) -> int {
            KvCopyJob j = shape, none;
            j.src = sd[(size_t)c]; j.dst = dd[(size_t)c];
            return launch_kv_copy(B.L, j, none);
        };
        FL_TRY(make(0));
        FL_TRY(op_run(B, sbytes + dbytes, iters, ms_out, make, run));
        FL_HIP(hipMemcpy(dst, dd[0], dbytes, hipMemcpyDeviceToHost));
        return FL_OK;
    });
}

int fl_op_attention(const void *q, const void *k, const void *v, int64_t T, int64_t s_past, int64_t H, int64_t Hkv, int64_t d,
                    int64_t window, int32_t kernel, int32_t nsplit, float *out) {
    return guarded([&]() -> int {
        if (!q || !k || !v || !out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument");
        if (T < 1 || s_past < 0 || H < 1 || Hkv < 1 || kernel < 0 || kernel > 3 || nsplit < 0 || nsplit > 64) FL_FAIL(FL_ERR_BAD_ARGUMENT, "bad shape / kernel");
        if (!attn_mfma_supported(FL_DTYPE_BF16, H, Hkv, d)) FL_FAIL(FL_ERR_UNSUPPORTED, "MFMA attention: head_dim 64 / 128, at most 8 query heads per kv head");
        if (kernel == 1 && T != 1) FL_FAIL(FL_ERR_BAD_ARGUMENT, "the decode kernel takes one query token");
        OpScope B;
        FL_TRY(B.begin());
        const int64_t S = s_past + T, sa = (S + 31) / 32 * 32;
        const size_t qn = (size_t)T * H * d;
        if (nsplit == 0) nsplit = (int)std::max<int64_t>(1, std::min<int64_t>((S + 127) / 128, 48));
        void *qd, *od, *kd, *vd; StepState *std_; float *pm, *pl, *po; unsigned *cnt;
        FL_TRY(B.upload(&qd, q, qn * 2));
        FL_TRY(B.alloc(&od, qn * 2));
        FL_HIP(hipMemset(od, 0xff, qn * 2));                      // NaN pattern: an element the kernel does not write shows up
        // the cache layout of the model: K [Hkv][sa][d], V transposed [Hkv][d][sa], zero padding
        FL_TRY(attn_op_upload_cache(B, &kd, &vd, FL_DTYPE_BF16, k, v, 1, S, Hkv, sa, d, true, 0.f));
        FL_TRY(attn_op_scratch(B, &pm, &pl, &po, &cnt, H, d, nsplit));
        StepState st{}; st.pos = (uint32_t)s_past; st.len = (uint32_t)s_past; st.call0 = (uint32_t)s_past; st.eos = -1;
        FL_TRY(B.upload(&std_, &st, sizeof st));
        const float scale = 1.0f / sqrtf((float)d);
        int rc;
        if (kernel == 1 || (kernel == 0 && T == 1)) {
            AttnScratch as{pm, pl, po, cnt, nsplit, S};
            rc = launch_attn_decode_mfma(B.L, qd, kd, vd, std_, od, as, H, Hkv, d, sa, scale);
        } else {
            attn_prefill_force(kernel);
            rc = launch_attn_prefill_mfma(B.L, qd, kd, vd, std_, od, T, H, Hkv, d, sa, scale, window < 0 ? -1 : window);
            attn_prefill_force(0);
        }
        FL_TRY(rc);
        FL_HIP(hipStreamSynchronize(B.s));
        return op_download(out, od, qn, FL_DTYPE_BF16);
    });
}

int fl_op_attention_plain(const void *q, const void *k, const void *v, int32_t dtype, int32_t layout, int32_t kernel, int64_t T, int64_t s_past,
                          int64_t call0, int64_t k_rows, int64_t capacity, int64_t H, int64_t Hkv, int64_t d, int64_t window, int32_t nsplit,
                          float pad_value, int32_t repeat, float *out) {
    return guarded([&]() -> int {
        if (!q || !k || !v || !out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument");
        if (T < 1 || s_past < 0 || call0 < 0 || call0 > s_past || kernel < 0 || kernel > 3 || (layout == 0 && kernel == 3) || nsplit < 0 || nsplit > 64 ||
            repeat < 1 || repeat > 16)
            FL_FAIL(FL_ERR_BAD_ARGUMENT, "bad shape / kernel (call0 <= s_past, nsplit 0..64, repeat 1..16; the plain layout has one prefill kernel)");
        if (kernel == 1 && T != 1) FL_FAIL(FL_ERR_BAD_ARGUMENT, "the decode kernel takes one query token");
        const int64_t S = s_past + T;
        if (k_rows < S || capacity < k_rows || capacity > (int64_t)1 << 24) FL_FAIL(FL_ERR_BAD_ARGUMENT, "s_past + T <= k_rows <= capacity");
        if (!(pad_value == pad_value) || pad_value - pad_value != 0.f) FL_FAIL(FL_ERR_BAD_ARGUMENT, "pad_value must be finite");
        FL_TRY(attn_op_check_heads(dtype, layout, H, Hkv, d));
        OpScope B;
        FL_TRY(B.begin());
        const bool mfma = layout == 1, decode = kernel == 1 || (kernel == 0 && T == 1);
        const int64_t sa = (capacity + 31) / 32 * 32;
        const size_t es = dtype == FL_DTYPE_BF16 ? 2 : 4, qn = (size_t)T * H * d;
        if (nsplit == 0) nsplit = attn_cache_nsplit(mfma, (size_t)capacity, d);
        void *qd, *od, *kd, *vd; StepState *std_; float *pm, *pl, *po; unsigned *cnt;
        FL_TRY(B.upload(&qd, q, qn * es));
        FL_TRY(B.alloc(&od, qn * es * repeat));
        FL_HIP(hipMemset(od, 0xff, qn * es * repeat));            // NaN pattern: an element a launch does not write shows up
        FL_TRY(attn_op_upload_cache(B, &kd, &vd, dtype, k, v, 1, k_rows, Hkv, sa, d, mfma, pad_value));
        FL_TRY(attn_op_scratch(B, &pm, &pl, &po, &cnt, H, d, nsplit));
        StepState st{}; st.pos = (uint32_t)s_past; st.len = (uint32_t)s_past; st.call0 = (uint32_t)call0; st.eos = -1;
        FL_TRY(B.upload(&std_, &st, sizeof st));
        const float scale = 1.0f / sqrtf((float)d);
        const int64_t w = window < 0 ? -1 : window;
        for (int r = 0; r < repeat; r++) {                          // every launch on the same scratch and ticket words
            void *o = (char *)od + (size_t)r * qn * es;
            int rc;
            if (decode) {
                AttnScratch as{pm, pl, po, cnt, nsplit, S};
                rc = mfma ? launch_attn_decode_mfma(B.L, qd, kd, vd, std_, o, as, H, Hkv, d, sa, scale)
                          : launch_attn_decode(B.L, dtype, qd, kd, vd, std_, o, as, H, Hkv, d, sa, scale);
            } else if (mfma) {
                attn_prefill_force(kernel);
                rc = launch_attn_prefill_mfma(B.L, qd, kd, vd, std_, o, T, H, Hkv, d, sa, scale, w);
                attn_prefill_force(0);
            } else {
                rc = launch_attn_prefill(B.L, dtype, qd, kd, vd, std_, o, T, H, Hkv, d, sa, scale, w);
            }
            FL_TRY(rc);
        }
        FL_HIP(hipStreamSynchronize(B.s));
        return op_download(out, od, qn * repeat, dtype);
    });
}

int fl_op_attention_batch(const void *q, const void *const *k, const void *const *v, int32_t dtype, int32_t layout, int64_t B_, const int64_t *lens,
                          const int64_t *k_rows, const int64_t *seq_alloc, const int32_t *nsplit, int64_t n_layers, int64_t layer, int64_t H,
                          int64_t Hkv, int64_t d, float pad_value, int32_t repeat, float *out) {
    return guarded([&]() -> int {
        if (!q || !k || !v || !lens || !k_rows || !seq_alloc || !nsplit || !out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument");
        if (B_ < 1 || B_ > 1023 || n_layers < 1 || n_layers > 64 || layer < 0 || layer >= n_layers || repeat < 1 || repeat > 16)
            FL_FAIL(FL_ERR_BAD_ARGUMENT, "bad shape (1 <= B <= 1023, layer < n_layers <= 64, repeat 1..16)");
        for (int64_t b = 0; b < B_; b++) {
            if (!k[b] || !v[b]) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument (sequence %lld)", (long long)b);
            if (lens[b] < 1 || k_rows[b] < lens[b] || seq_alloc[b] < k_rows[b] || seq_alloc[b] % 32 != 0 || seq_alloc[b] > (int64_t)1 << 24)
                FL_FAIL(FL_ERR_BAD_ARGUMENT, "sequence %lld: 1 <= len <= k_rows <= seq_alloc, seq_alloc a multiple of 32", (long long)b);
            if (nsplit[b] < 0 || nsplit[b] > 64) FL_FAIL(FL_ERR_BAD_ARGUMENT, "sequence %lld: nsplit 0..64", (long long)b);
        }
        if (!(pad_value == pad_value) || pad_value - pad_value != 0.f) FL_FAIL(FL_ERR_BAD_ARGUMENT, "pad_value must be finite");
        FL_TRY(attn_op_check_heads(dtype, layout, H, Hkv, d));
        OpScope B;
        FL_TRY(B.begin());
        const bool mfma = layout == 1;
        const int nb = (int)B_;
        const size_t es = dtype == FL_DTYPE_BF16 ? 2 : 4, qn = (size_t)nb * H * d;
        void *qd, *od;
        FL_TRY(B.upload(&qd, q, qn * es));
        FL_TRY(B.alloc(&od, qn * es * repeat));
        FL_HIP(hipMemset(od, 0xff, qn * es * repeat));
        // every sequence a cache of its own, as fl_batch_create finds them: K / V of all layers, step state, split scratch, ticket
        // words; the SeqRef fields the attention kernels do not read stay null
        std::vector<SeqRef> refs((size_t)nb);
        int max_nsplit = 1;
        for (int b = 0; b < nb; b++) {
            SeqRef &r = refs[(size_t)b];
            r = SeqRef{};
            r.seq_alloc = (int)seq_alloc[b];
            r.nsplit = nsplit[b] > 0 ? nsplit[b] : attn_cache_nsplit(mfma, (size_t)seq_alloc[b], d);
            max_nsplit = std::max(max_nsplit, r.nsplit);
            FL_TRY(attn_op_upload_cache(B, &r.k, &r.v, dtype, k[b], v[b], n_layers, k_rows[b], Hkv, seq_alloc[b], d, mfma, pad_value));
            FL_TRY(attn_op_scratch(B, &r.part_m, &r.part_l, &r.part_o, &r.counters, H, d, r.nsplit));
            StepState st{}; st.pos = (uint32_t)(lens[b] - 1); st.len = (uint32_t)(lens[b] - 1); st.call0 = st.len; st.eos = -1;
            FL_TRY(B.upload(&r.st, &st, sizeof st));
        }
        SeqRef *seqs_dev;
        FL_TRY(B.upload(&seqs_dev, refs.data(), sizeof(SeqRef) * (size_t)nb));
        const float scale = 1.0f / sqrtf((float)d);
        const size_t kv_layer_off = (size_t)(layer * Hkv * d);
        for (int r = 0; r < repeat; r++) {
            void *o = (char *)od + (size_t)r * qn * es;
            if (mfma) FL_TRY(launch_attn_decode_mfma_batch(B.L, qd, seqs_dev, nb, max_nsplit, kv_layer_off, o, H, Hkv, d, scale, 0.0));
            else FL_TRY(launch_attn_decode_batch(B.L, dtype, qd, seqs_dev, nb, max_nsplit, kv_layer_off, o, H, Hkv, d, scale));
        }
        FL_HIP(hipStreamSynchronize(B.s));
        return op_download(out, od, qn * repeat, dtype);
    });
}

int fl_op_attention_packed(const void *q, const void *const *k, const void *const *v, int64_t n_seq, const int64_t *offsets, const int64_t *s_past,
                           const int64_t *k_rows, const int64_t *seq_alloc, int64_t n_layers, int64_t layer, int64_t H, int64_t Hkv, int64_t d,
                           int64_t window, float pad_value, float *out) {
    return fl_op_attention_packed_ex(q, k, v, n_seq, offsets, s_past, k_rows, seq_alloc, n_layers, layer, H, Hkv, d, window, pad_value, FL_MASK_CAUSAL, out);
}

int fl_op_attention_packed_ex(const void *q, const void *const *k, const void *const *v, int64_t n_seq, const int64_t *offsets, const int64_t *s_past,
                              const int64_t *k_rows, const int64_t *seq_alloc, int64_t n_layers, int64_t layer, int64_t H, int64_t Hkv, int64_t d,
                              int64_t window, float pad_value, int32_t mask, float *out) {
    return guarded([&]() -> int {
        if (mask != FL_MASK_CAUSAL && mask != FL_MASK_FULL) FL_FAIL(FL_ERR_BAD_ARGUMENT, "mask %d is neither FL_MASK_CAUSAL nor FL_MASK_FULL", mask);
        if (!q || !k || !v || !offsets || !s_past || !k_rows || !seq_alloc || !out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument");
        if (n_seq < 1 || n_seq > 1023 || n_layers < 1 || n_layers > 64 || layer < 0 || layer >= n_layers)
            FL_FAIL(FL_ERR_BAD_ARGUMENT, "bad shape (1 <= n_seq <= 1023, layer < n_layers <= 64)");
        if (offsets[0] != 0) FL_FAIL(FL_ERR_BAD_ARGUMENT, "offsets[0] must be 0");
        for (int64_t s = 0; s < n_seq; s++) {
            if (!k[s] || !v[s]) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument (sequence %lld)", (long long)s);
            const int64_t cnt = offsets[s + 1] - offsets[s];
            if (cnt < 1 || cnt > (int64_t)1 << 24 || s_past[s] < 0 || s_past[s] > (int64_t)1 << 24) FL_FAIL(FL_ERR_BAD_ARGUMENT, "sequence %lld: at least one new token, s_past >= 0", (long long)s);
            if (k_rows[s] < s_past[s] + cnt || seq_alloc[s] < k_rows[s] || seq_alloc[s] % 32 != 0 || seq_alloc[s] > (int64_t)1 << 24)
                FL_FAIL(FL_ERR_BAD_ARGUMENT, "sequence %lld: s_past + new tokens <= k_rows <= seq_alloc, seq_alloc a multiple of 32", (long long)s);
        }
        if (offsets[n_seq] > (int64_t)1 << 24) FL_FAIL(FL_ERR_BAD_ARGUMENT, "too many rows");
        if (!(pad_value == pad_value) || pad_value - pad_value != 0.f) FL_FAIL(FL_ERR_BAD_ARGUMENT, "pad_value must be finite");
        FL_TRY(attn_op_check_heads(FL_DTYPE_BF16, 1, H, Hkv, d));
        OpScope B;
        FL_TRY(B.begin());
        const int ns = (int)n_seq;
        const size_t qn = (size_t)offsets[n_seq] * H * d;
        void *qd, *od;
        FL_TRY(B.upload(&qd, q, qn * 2));
        FL_TRY(B.alloc(&od, qn * 2));
        FL_HIP(hipMemset(od, 0xff, qn * 2));                      // NaN pattern: an element the kernel does not write shows up
        // every sequence a cache of its own, as fl_batch_prefill finds them: K / V^T of all layers and the step state of the call
        std::vector<SeqRef> refs((size_t)ns);
        std::vector<int> counts((size_t)ns), vt((size_t)ns, 1);
        for (int s = 0; s < ns; s++) {
            SeqRef &r = refs[(size_t)s];
            r = SeqRef{};
            r.seq_alloc = (int)seq_alloc[s]; r.nsplit = 1;
            counts[(size_t)s] = (int)(offsets[s + 1] - offsets[s]);
            FL_TRY(attn_op_upload_cache(B, &r.k, &r.v, FL_DTYPE_BF16, k[s], v[s], n_layers, k_rows[s], Hkv, seq_alloc[s], d, true, pad_value));
            StepState st{}; st.pos = (uint32_t)s_past[s]; st.len = (uint32_t)s_past[s]; st.call0 = st.len; st.eos = -1;
            FL_TRY(B.upload(&r.st, &st, sizeof st));
        }
        PackedHost ph;
        packed_table_build(refs.data(), counts.data(), vt.data(), ns, H, Hkv, d, &ph);
        void *tabd;
        FL_TRY(B.upload(&tabd, ph.bytes.data(), ph.bytes.size()));
        const float scale = 1.0f / sqrtf((float)d);
        FL_TRY(launch_attn_prefill_packed_mfma(B.L, qd, ph.at(tabd), ph.n_items, ph.TT, ph.ks, (size_t)(layer * Hkv * d), od, H, Hkv, d, scale, window < 0 ? -1 : window, 0, mask));
        FL_HIP(hipStreamSynchronize(B.s));
        return op_download(out, od, qn, FL_DTYPE_BF16);
    });
}

// ---- the pooling op: fl_batch_embed's pool launch on host rows --------------------------------------------------------------------

namespace {
struct PoolOp { float *xd, *id, *wd, *part, *od; int *off, *cnt; int n_out, T; int64_t dims; };

int pool_op_setup(OpScope &B, const char *who, const float *x, const float *inv_rms, const float *w, const size_t *offsets, size_t n_seq, int64_t h,
                  const fl_embed *opts, PoolOp *p) {
    FL_TRY(check_embed(opts, 0));
    if (!x || !inv_rms || !w || !offsets) FL_FAIL(FL_ERR_BAD_ARGUMENT, "%s: null argument", who);
    if (h < 1 || h > 65536) FL_FAIL(FL_ERR_BAD_ARGUMENT, "%s: h %lld not in 1..65536", who, (long long)h);
    FL_TRY(check_embed(opts, h));
    if (n_seq < 1 || n_seq > ((size_t)1 << 20) || offsets[0] != 0) FL_FAIL(FL_ERR_BAD_ARGUMENT, "%s: 1 <= n_seq <= 2^20, offsets[0] == 0", who);
    for (size_t s = 0; s < n_seq; s++)
        if (offsets[s + 1] <= offsets[s] || offsets[s + 1] > ((size_t)1 << 20)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "%s: offsets must increase, up to T <= 2^20", who);
    const size_t T = offsets[n_seq];
    p->T = (int)T;
    p->dims = opts->dimensions ? opts->dimensions : h;
    p->n_out = opts->pooling == FL_POOL_NONE ? (int)T : (int)n_seq;
    std::vector<int> off(n_seq), cnt(n_seq);
    for (size_t s = 0; s < n_seq; s++) { off[s] = (int)offsets[s]; cnt[s] = (int)(offsets[s + 1] - offsets[s]); }
    FL_TRY(B.begin());
    FL_TRY(B.upload(&p->xd, x, T * (size_t)h * 4));
    FL_TRY(B.upload(&p->id, inv_rms, T * 4));
    FL_TRY(B.upload(&p->wd, w, (size_t)h * 4));
    FL_TRY(B.upload(&p->off, off.data(), n_seq * 4));
    FL_TRY(B.upload(&p->cnt, cnt.data(), n_seq * 4));
    FL_TRY(B.alloc(&p->part, (size_t)p->n_out * pool_rows_chunks(p->dims) * 4));
    FL_TRY(B.alloc(&p->od, (size_t)p->n_out * p->dims * 4));
    return FL_OK;
}
}  // namespace

int fl_op_pool_rows(const float *x, const float *inv_rms, const float *w, const size_t *offsets, size_t n_seq, int64_t h, const fl_embed *opts,
                    float *out) {
    return guarded([&]() -> int {
        if (!out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_pool_rows: null out");
        OpScope B;
        PoolOp p{};
        FL_TRY(pool_op_setup(B, "fl_op_pool_rows", x, inv_rms, w, offsets, n_seq, h, opts, &p));
        const size_t bytes = (size_t)p.n_out * p.dims * 4;
        std::vector<float> host[2];
        for (int rep = 0; rep < 2; rep++) {                     // twice: the same launch must give the same bits
            host[rep].resize(bytes / 4);
            FL_HIP(hipMemsetAsync(p.od, 0xff, bytes, B.s));      // NaN pattern: an element the kernel does not write shows up
            FL_TRY(launch_pool_rows(B.L, p.xd, p.id, p.wd, p.off, p.cnt, p.n_out, h, p.dims, opts->pooling, opts->normalize != 0, p.part, p.od));
            FL_HIP(hipStreamSynchronize(B.s));
            FL_HIP(hipMemcpy(host[rep].data(), p.od, bytes, hipMemcpyDeviceToHost));
        }
        if (memcmp(host[0].data(), host[1].data(), bytes)) FL_FAIL(FL_ERR_HIP, "pool_rows: a repeated launch gave another result");
        memcpy(out, host[0].data(), bytes);
        return FL_OK;
    });
}

int fl_op_pool_rows_time(const float *x, const float *inv_rms, const float *w, const size_t *offsets, size_t n_seq, int64_t h, const fl_embed *opts,
                         int32_t iters, double *ms_out) {
    return guarded([&]() -> int {
        if (!ms_out || iters < 1 || iters > (1 << 20)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_pool_rows_time: null ms_out or a bad iteration count");
        OpScope B;
        PoolOp p{};
        FL_TRY(pool_op_setup(B, "fl_op_pool_rows_time", x, inv_rms, w, offsets, n_seq, h, opts, &p));
        auto run = [&]() { return launch_pool_rows(B.L, p.xd, p.id, p.wd, p.off, p.cnt, p.n_out, h, p.dims, opts->pooling, opts->normalize != 0, p.part, p.od); };
        FL_TRY(run());                                           // warm
        FL_HIP(hipStreamSynchronize(B.s));
        FL_HIP(hipEventCreate(&B.e0)); FL_HIP(hipEventCreate(&B.e1));
        FL_HIP(hipEventRecord(B.e0, B.s));
        for (int i = 0; i < iters; i++) FL_TRY(run());
        FL_HIP(hipEventRecord(B.e1, B.s));
        FL_HIP(hipEventSynchronize(B.e1));
        float ms = 0.f; FL_HIP(hipEventElapsedTime(&ms, B.e0, B.e1));
        *ms_out = ms / iters;
        return FL_OK;
    });
}

int fl_op_rmsnorm_add(float *x_res, const float *delta, int32_t n_slab, const float *w, float eps, int64_t T, int64_t h, int32_t dtype,
                      float *xs_out, float *inv_rms_out) {
    return guarded([&]() -> int {
        if (!x_res || !w || !xs_out || !inv_rms_out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument");
        if (dtype != FL_DTYPE_BF16 && dtype != FL_DTYPE_F32) FL_FAIL(FL_ERR_UNSUPPORTED, "dtype must be bf16 or f32");
        if (T <= 0 || T > (1 << 20) || h <= 0 || h % 8) FL_FAIL(FL_ERR_BAD_ARGUMENT, "bad shape (h must be a multiple of 8)");
        if (n_slab < 0 || n_slab > 64 || (n_slab > 0) != (delta != nullptr)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "n_slab 0..64, with delta exactly when it is not 0");
        OpScope B;
        FL_TRY(B.begin());
        const size_t n = (size_t)T * h, es = dtype == FL_DTYPE_BF16 ? 2 : 4;
        float *xd, *dd = nullptr, *wd, *inv; void *xs;
        FL_TRY(B.upload(&xd, x_res, n * 4));
        if (delta) FL_TRY(B.upload(&dd, delta, n * 4 * n_slab));
        FL_TRY(B.upload(&wd, w, (size_t)h * 4));
        FL_TRY(B.alloc(&xs, n * es));
        FL_TRY(B.alloc(&inv, (size_t)T * 4));
        FL_HIP(hipMemset(xs, 0xff, n * es));                       // NaN pattern: an element the kernel does not write shows up
        FL_HIP(hipMemset(inv, 0xff, (size_t)T * 4));
        FL_TRY(launch_rmsnorm_add(B.L, dtype, xd, dd, wd, eps, xs, inv, T, h, std::max(n_slab, 1), (int64_t)n));
        FL_HIP(hipStreamSynchronize(B.s));
        FL_HIP(hipMemcpy(x_res, xd, n * 4, hipMemcpyDeviceToHost));
        FL_HIP(hipMemcpy(inv_rms_out, inv, (size_t)T * 4, hipMemcpyDeviceToHost));
        return op_download(xs_out, xs, n, dtype);
    });
}

int fl_op_norm_linear(const fl_norm_linear_args *args) {
    return guarded([&]() -> int {
        FL_TRY(norm_linear_check(args));
        const fl_norm_linear_args &a = *args;
        OpScope B;
        FL_TRY(B.begin());
        const int dtype = a.dtype, epi = a.epilogue, form = a.form;
        const int64_t T = a.T, N = a.N, K = a.K, I = N / 2;
        const size_t es = dtype == FL_DTYPE_BF16 ? 2 : 4, nx = (size_t)T * K;
        const bool norm = a.pro == PRO_NORM;
        // the weights: e4m3 bytes + row scales (form 2), else a matrix of the compute dtype
        int64_t Nw = N, Ip = (I + 15) / 16 * 16;
        void *wd = nullptr; float *sd = nullptr, *bd = nullptr;
        if (form == 2) {
            Nw = epi == EPI_GATEUP ? 2 * Ip : N;
            if (epi == EPI_GATEUP) {
                uint8_t *qs, *qd; float *ss;
                FL_TRY(B.upload(&qs, a.w, (size_t)N * K));
                FL_TRY(B.upload(&ss, a.w_scale, (size_t)N * 4));
                FL_TRY(B.alloc(&qd, (size_t)Nw * K));
                FL_TRY(B.alloc(&sd, (size_t)Nw * 4));
                FL_HIP(hipMemsetAsync(qd, 0, (size_t)Nw * K, B.s));
                FL_HIP(hipMemsetAsync(sd, 0, (size_t)Nw * 4, B.s));
                FL_TRY(launch_w8_gateup_layout(B.L, qs, ss, I, K, qd, sd));
                wd = qd;
            } else {
                FL_TRY(B.upload(&wd, a.w, (size_t)N * K));
                FL_TRY(B.upload(&sd, a.w_scale, (size_t)N * 4));
            }
        } else {
            FL_TRY(op_upload_matrix(B, dtype, a.w, N, K, epi, &wd, &Nw, &Ip));
        }
        if (a.bias) FL_TRY(B.upload(&bd, a.bias, (size_t)N * 4));
        const int64_t Ny = epi == EPI_GATEUP ? Ip : N;               // columns of the device output
        const size_t ybytes = (size_t)T * Ny * (epi == EPI_GATEUP ? es : 4);
        // the norm's inputs: the residual rows (a pristine copy: form 0 updates them in place), or the embedding matrix and one
        // step state per row holding its token
        float *xr0 = nullptr, *xr = nullptr, *xo = nullptr, *dd = nullptr, *nw = nullptr, *inv = nullptr;
        void *xs = nullptr, *xp = nullptr, *ed = nullptr; uint32_t *ids = nullptr; StepState *std_ = nullptr; SeqRef *seqs = nullptr;
        if (norm) {
            FL_TRY(B.upload(&nw, a.norm_w, (size_t)K * 4));
            FL_TRY(B.alloc(&xo, nx * 4));
            if (a.delta) FL_TRY(B.upload(&dd, a.delta, nx * 4 * a.n_slab));
            if (a.embed) {
                FL_TRY(B.upload(&ed, a.embed, (size_t)a.vocab * K * es));
                FL_TRY(B.upload(&ids, a.tokens, (size_t)T * 4));
                std::vector<StepState> st((size_t)T);
                std::vector<SeqRef> refs((size_t)T);
                for (int64_t t = 0; t < T; t++) { st[(size_t)t] = StepState{}; st[(size_t)t].token = a.tokens[t]; st[(size_t)t].eos = -1; }
                FL_TRY(B.upload(&std_, st.data(), sizeof(StepState) * (size_t)T));
                for (int64_t t = 0; t < T; t++) { refs[(size_t)t] = SeqRef{}; refs[(size_t)t].st = std_ + t; }
                FL_TRY(B.upload(&seqs, refs.data(), sizeof(SeqRef) * (size_t)T));
            } else {
                FL_TRY(B.upload(&xr0, a.x_res, nx * 4));
            }
            if (form == 0) {
                FL_TRY(B.alloc(&xr, nx * 4));
                FL_TRY(B.alloc(&xs, nx * es));
                FL_TRY(B.alloc(&inv, (size_t)T * 4));
            }
        } else {
            FL_TRY(B.upload(&xp, a.x, nx * 2));
        }
        // form 0: K slabs as fl_op_linear allows them, and its FL_OP_LINEAR_DMA route; form 3: the batched stream's K slices
        const int op_split = tune(TK_OP_MAXSPLIT);
        const int max_split = form == 0 && epi == EPI_F32 && !bd ? (op_split > 0 ? op_split : std::max(4, ksplit_cap(T))) : 1;
        const int nks = form == 3 ? gemv_batch_ksplit((int)T, K, Nw, epi) : 1;
        const bool dma = form == 0 && tune(TK_OP_LINEAR_DMA) == 1 && dtype == FL_DTYPE_BF16 && T <= 32 && !bd && gemv_dma_supported((int)T, Nw, K, epi, 0) &&
                         gemv_dma_ksplit(K, Nw, epi) <= max_split;
        int nsplit = 1;
        void *yd;
        FL_TRY(B.alloc(&yd, ybytes * std::max(max_split, nks)));
        if (a.kernels_out) {
            const LinearPlan p = form == 0 ? plan_linear(dtype, T, Nw, K, epi, B.L.tp, max_split, bd != nullptr, true, false) : LinearPlan{};
            a.kernels_out[0] = dma ? (int)LK_DMA : p.kernel; a.kernels_out[1] = form == 3 ? nks : dma ? gemv_dma_ksplit(K, Nw, epi) : p.ks;
            a.kernels_out[2] = dma ? (int)LK_NONE : p.tail; a.kernels_out[3] = dma ? (int)LK_NONE : p.rest;
        }
        auto run = [&]() -> int {
            FL_HIP(hipMemsetAsync(yd, 0xff, ybytes * std::max(max_split, nks), B.s));      // NaN pattern: an element no launch writes shows up
            if (xo) FL_HIP(hipMemsetAsync(xo, 0xff, nx * 4, B.s));
            if (form == 0) {
                if (a.embed) FL_TRY(launch_embed(B.L, dtype, ed, ids, nullptr, xr, T, K));
                else FL_HIP(hipMemcpyAsync(xr, xr0, nx * 4, hipMemcpyDeviceToDevice, B.s));
                FL_TRY(launch_rmsnorm_add(B.L, dtype, xr, dd, nw, a.eps, xs, inv, T, K, std::max(a.n_slab, 1), (int64_t)nx));
                if (!dma) return launch_linear(B.L, dtype, wd, xs, bd, yd, T, Nw, K, epi, inv, max_split, &nsplit);
                GemvBatchArgs ga;
                ga.W = wd; ga.x = xs; ga.x_scale = inv; ga.out = yd; ga.N = (int)Nw; ga.K = (int)K; ga.epi = epi; ga.pro = PRO_X; ga.B = (int)T;
                ga.nks = epi == EPI_F32 ? gemv_dma_ksplit(K, Nw, epi) : 1;
                nsplit = ga.nks;
                return launch_gemv_dma(B.L, ga);
            }
            if (form == 3) {
                GemvBatchArgs ga;
                ga.W = wd; ga.bias = bd; ga.out = yd; ga.N = (int)Nw; ga.K = (int)K; ga.epi = epi; ga.pro = a.pro; ga.B = (int)T; ga.nks = nks;
                ga.x = xp; ga.x_in = xr0; ga.delta = dd; ga.norm_w = nw; ga.n_slab = std::max(a.n_slab, 1); ga.slab_stride = (long long)nx; ga.eps = a.eps;
                ga.x_out = xo; ga.embed = ed; ga.seqs = seqs;
                nsplit = nks;
                return launch_gemv_batch(B.L, ga);
            }
            GemvArgs ga;
            ga.W = wd; ga.bias = bd; ga.out = yd; ga.N = (int)Nw; ga.K = (int)K; ga.epi = epi; ga.pro = PRO_NORM;
            ga.x_in = xr0; ga.delta = dd; ga.delta_nslab = std::max(a.n_slab, 1); ga.norm_w = nw; ga.eps = a.eps; ga.x_out = xo; ga.embed = ed; ga.st = std_;
            return form == 1 ? launch_gemv(B.L, dtype, ga) : launch_gemv_w8(B.L, ga, sd);
        };
        std::vector<unsigned char> first, again;
        std::vector<float> xfirst(norm ? nx : 0), xagain(norm ? nx : 0);
        for (int rep = 0; rep < a.repeat; rep++) {
            FL_TRY(run());
            FL_HIP(hipStreamSynchronize(B.s));
            std::vector<unsigned char> &yb = rep ? again : first;
            std::vector<float> &xb = rep ? xagain : xfirst;
            yb.resize(ybytes * (size_t)nsplit);
            FL_HIP(hipMemcpy(yb.data(), yd, yb.size(), hipMemcpyDeviceToHost));
            if (norm) FL_HIP(hipMemcpy(xb.data(), form == 0 ? xr : xo, nx * 4, hipMemcpyDeviceToHost));
            if (rep && (first != again || (norm && memcmp(xfirst.data(), xagain.data(), nx * 4))))
                FL_FAIL(FL_ERR_HIP, "fl_op_norm_linear: launch %d of form %d gave another result than the first", rep, form);
        }
        if (a.x_out && norm) memcpy(a.x_out, xfirst.data(), nx * 4);
        if (epi == EPI_GATEUP) {                                     // without the padding columns
            for (int64_t t = 0; t < T; t++)
                for (int64_t j = 0; j < I; j++) {
                    const size_t idx = (size_t)(t * Ip + j);
                    a.y[t * I + j] = es == 2 ? bf16_bits_to_float(reinterpret_cast<const bf16_t *>(first.data())[idx]) : reinterpret_cast<const float *>(first.data())[idx];
                }
            return FL_OK;
        }
        const float *slabs = reinterpret_cast<const float *>(first.data());
        for (size_t i = 0; i < (size_t)T * N; i++) {                 // the K slabs summed in slab order, like rmsnorm_add does
            float s = slabs[i];
            for (int sl = 1; sl < nsplit; sl++) s += slabs[(size_t)sl * T * N + i];
            a.y[i] = s;
        }
        return FL_OK;
    });
}

int fl_op_linear_resid(const fl_linear_resid_args *args) {
    return guarded([&]() -> int {
        if (!args) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_linear_resid: null args");
        const fl_linear_resid_args &a = *args;
        if (a.struct_size != sizeof(fl_linear_resid_args)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_linear_resid: struct_size %zu, expected %zu", a.struct_size, sizeof(fl_linear_resid_args));
        if (!a.x || !a.w || !a.h_in || !a.w_next || !a.h_out || !a.xn_out || !a.inv_rms_out || !a.part_out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "null argument");
        if (a.T <= 0 || a.N <= 0 || a.K <= 0 || a.K % 8 || a.N % 8) FL_FAIL(FL_ERR_BAD_ARGUMENT, "bad shape (N and K must be multiples of 8)");
        if (a.repeat < 1 || a.repeat > 8) FL_FAIL(FL_ERR_BAD_ARGUMENT, "repeat %d not in 1..8", a.repeat);
        if (a.w2 && (!a.y2_out || a.N2 <= 0 || (a.epi2 != EPI_F32 && a.epi2 != EPI_GATEUP) || (a.epi2 == EPI_GATEUP && a.N2 % 2)))
            FL_FAIL(FL_ERR_BAD_ARGUMENT, "the consumer: y2_out, N2 > 0 (even for gate/up), epi2 0 or 1");
        OpScope B;
        FL_TRY(B.begin());
        const int64_t T = a.T, N = a.N, K = a.K;
        const LinearPlan p = plan_resid(FL_DTYPE_BF16, T, N, K, ksplit_cap(T), false);
        if (p.kernel == LK_NONE) FL_FAIL(FL_ERR_UNSUPPORTED, "fl_op_linear_resid: no kernel takes the residual epilogue at T %lld, N %lld, K %lld", (long long)T, (long long)N, (long long)K);
        const int np = gemm_resid_partials(N);
        const size_t nh = (size_t)T * N, npart = (size_t)T * np;
        void *xd, *wd, *xn, *w2d = nullptr, *y2 = nullptr; float *bd = nullptr, *h0, *h, *wn, *part, *inv;
        FL_TRY(B.upload(&xd, a.x, (size_t)T * K * 2));
        FL_TRY(B.upload(&wd, a.w, (size_t)N * K * 2));
        if (a.bias) FL_TRY(B.upload(&bd, a.bias, (size_t)N * 4));
        FL_TRY(B.upload(&h0, a.h_in, nh * 4));
        FL_TRY(B.upload(&wn, a.w_next, (size_t)N * 4));
        FL_TRY(B.alloc(&h, nh * 4));
        FL_TRY(B.alloc(&xn, nh * 2));
        FL_TRY(B.alloc(&part, npart * 4));
        FL_TRY(B.alloc(&inv, (size_t)T * 4));
        int64_t N2w = 0, I2p = 0;
        size_t y2bytes = 0;
        LinearPlan cp;
        if (a.w2) {
            FL_TRY(op_upload_matrix(B, FL_DTYPE_BF16, a.w2, a.N2, N, a.epi2, &w2d, &N2w, &I2p));
            y2bytes = a.epi2 == EPI_GATEUP ? (size_t)T * I2p * 2 : (size_t)T * a.N2 * 4;
            FL_TRY(B.alloc(&y2, y2bytes));
            cp = plan_linear(FL_DTYPE_BF16, T, N2w, N, a.epi2, B.L.tp, 1, false, false, false);
        }
        if (a.kernels_out) {
            a.kernels_out[0] = p.kernel; a.kernels_out[1] = p.ks; a.kernels_out[2] = p.n_main < N ? p.tail : (int)LK_NONE; a.kernels_out[3] = p.tail_ks;
            a.kernels_out[4] = cp.kernel; a.kernels_out[5] = cp.reads_rs_parts ? 1 : 0;
        }
        ResidEpi re;                                                 // as resid_epi (model.hip) lays it out
        re.h = h; re.w = wn; re.xn = xn; re.part = part; re.np = np;
        // what one launch sequence left, as bytes: h | xn | part | y2 | inv
        const size_t off_xn = nh * 4, off_part = off_xn + nh * 2, off_y2 = off_part + npart * 4, off_inv = off_y2 + y2bytes, total = off_inv + (size_t)T * 4;
        std::vector<unsigned char> first(total), again(total);
        for (int rep = 0; rep < a.repeat; rep++) {
            // NaN patterns: a slot, an element or a row scale nobody writes shows up
            FL_HIP(hipMemcpyAsync(h, h0, nh * 4, hipMemcpyDeviceToDevice, B.s));
            FL_HIP(hipMemsetAsync(xn, 0xff, nh * 2, B.s));
            FL_HIP(hipMemsetAsync(part, 0xff, npart * 4, B.s));
            FL_HIP(hipMemsetAsync(inv, 0xff, (size_t)T * 4, B.s));
            if (y2) FL_HIP(hipMemsetAsync(y2, 0xff, y2bytes, B.s));
            FL_TRY(launch_plan(B.L, p, FL_DTYPE_BF16, wd, xd, bd, nullptr, T, N, K, EPI_RESID, nullptr, &re));
            if (!a.lazy) FL_TRY(launch_rms_finalize(B.L, part, np, a.eps, inv, T, N));
            else if (a.w2) B.L.rsp = RsParts{part, np, a.eps, 1.0f / (float)N};          // what with_parts does in enqueue_forward
            if (a.w2) {
                const int rc = launch_linear(B.L, FL_DTYPE_BF16, w2d, xn, nullptr, y2, T, N2w, N, a.epi2, inv);
                B.L.rsp = RsParts{};
                FL_TRY(rc);
            }
            FL_HIP(hipStreamSynchronize(B.s));
            unsigned char *o = (rep ? again : first).data();
            FL_HIP(hipMemcpy(o, h, nh * 4, hipMemcpyDeviceToHost));
            FL_HIP(hipMemcpy(o + off_xn, xn, nh * 2, hipMemcpyDeviceToHost));
            FL_HIP(hipMemcpy(o + off_part, part, npart * 4, hipMemcpyDeviceToHost));
            if (y2) FL_HIP(hipMemcpy(o + off_y2, y2, y2bytes, hipMemcpyDeviceToHost));
            if (a.lazy && !a.w2) {                                   // nobody consumed the partial sums: the vector they finish into
                FL_TRY(launch_rms_finalize(B.L, part, np, a.eps, inv, T, N));
                FL_HIP(hipStreamSynchronize(B.s));
            }
            FL_HIP(hipMemcpy(o + off_inv, inv, (size_t)T * 4, hipMemcpyDeviceToHost));
            if (rep && first != again) FL_FAIL(FL_ERR_HIP, "fl_op_linear_resid: launch %d gave another result than the first", rep);
        }
        memcpy(a.h_out, first.data(), nh * 4);
        const bf16_t *xb = reinterpret_cast<const bf16_t *>(first.data() + off_xn);
        for (size_t i = 0; i < nh; i++) a.xn_out[i] = bf16_bits_to_float(xb[i]);
        memcpy(a.part_out, first.data() + off_part, npart * 4);
        memcpy(a.inv_rms_out, first.data() + off_inv, (size_t)T * 4);
        if (y2 && a.epi2 == EPI_GATEUP) {
            const bf16_t *yb = reinterpret_cast<const bf16_t *>(first.data() + off_y2);
            const int64_t I2 = a.N2 / 2;
            for (int64_t t = 0; t < T; t++)
                for (int64_t j = 0; j < I2; j++) a.y2_out[t * I2 + j] = bf16_bits_to_float(yb[t * I2p + j]);
        } else if (y2) {
            memcpy(a.y2_out, first.data() + off_y2, y2bytes);
        }
        return FL_OK;
    });
}

int fl_op_rope_kv(const fl_rope_kv_args *args) {
    return guarded([&]() -> int {
        int64_t rows = 0;
        FL_TRY(rope_kv_check(args, &rows));
        const fl_rope_kv_args &a = *args;
        const fl_rope_seqs &q = a.seqs;
        OpScope B;
        FL_TRY(B.begin());
        const int dtype = a.dtype, form = a.form;
        const int64_t H = a.H, Hkv = a.Hkv, d = a.d, N = (H + 2 * Hkv) * d;
        const size_t es = dtype == FL_DTYPE_BF16 ? 2 : 4, qbytes = (size_t)rows * H * d * es;
        float *qkv, *bd = nullptr, *ct, *sn; void *qd;
        FL_TRY(B.upload(&qkv, a.qkv, (size_t)a.n_slab * rows * N * 4));
        if (a.bias) FL_TRY(B.upload(&bd, a.bias, (size_t)N * 4));
        FL_TRY(B.upload(&ct, a.cos_tab, (size_t)a.max_pos * (d / 2) * 4));
        FL_TRY(B.upload(&sn, a.sin_tab, (size_t)a.max_pos * (d / 2) * 4));
        FL_TRY(B.alloc(&qd, qbytes));
        RopeSeqsDev sq;
        FL_TRY(sq.upload(B, q, Hkv, d, es, nullptr));
        const size_t kv_layer_off = (size_t)q.layer * Hkv * d;       // times a sequence's seq_alloc: its layer, in elements
        const bool vt0 = q.v_transposed[0] != 0;
        const bool vec = form == 0 && rope_kv_takes_vec(dtype, vt0, rows, d, q.seq_alloc[0]);
        PackedHost ph;
        void *tabd = nullptr;
        if (form == 2) {
            std::vector<int> counts(q.count, q.count + q.n_seq), vt(q.n_seq);
            for (int s = 0; s < q.n_seq; s++) vt[(size_t)s] = q.v_transposed[s] ? 1 : 0;
            packed_table_build(sq.refs.data(), counts.data(), vt.data(), q.n_seq, H, Hkv, d, &ph);
            FL_TRY(B.upload(&tabd, ph.bytes.data(), ph.bytes.size()));
        }
        if (a.kernels_out) {
            a.kernels_out[0] = form == 0 ? (vec ? 1 : 0) : form + 1; a.kernels_out[1] = dtype; a.kernels_out[2] = form < 2 && vt0 ? 1 : 0;
            a.kernels_out[3] = vec ? (int)((rows * (H + Hkv) * (d / 16) + 255) / 256) : 0;
        }
        std::vector<unsigned char> first;
        FL_TRY(rope_op_repeat(B, "fl_op_rope_kv", sq, qd, qbytes, nullptr, 0, a.repeat, first, [&]() -> int {
            if (form == 0) {
                const size_t off = kv_layer_off * (size_t)q.seq_alloc[0] * es;
                return launch_rope_kv(B.L, dtype, qkv, sq.st, ct, sn, a.max_pos, qd, (char *)sq.k[0] + off, (char *)sq.v[0] + off, rows, H, Hkv, d, q.seq_alloc[0],
                                      vt0, a.n_slab, bd);
            }
            if (form == 1) return launch_rope_kv_batch(B.L, qkv, sq.refs_dev, ct, sn, a.max_pos, qd, kv_layer_off, q.n_seq, H, Hkv, d, a.n_slab, bd, dtype, vt0);
            return launch_rope_kv_packed(B.L, dtype, qkv, ph.at(tabd), ct, sn, a.max_pos, qd, kv_layer_off, rows, H, Hkv, d, a.n_slab, bd);
        }));
        memcpy(a.q_out, first.data(), qbytes);
        sq.give_back(q, first.data() + qbytes);
        return FL_OK;
    });
}

int fl_op_qkv_rope(const fl_qkv_rope_args *args) {
    return guarded([&]() -> int {
        FL_TRY(qkv_rope_check(args));
        const fl_qkv_rope_args &a = *args;
        const fl_rope_seqs &q = a.seqs;
        OpScope B;
        FL_TRY(B.begin());
        const int dtype = a.dtype, form = a.form;
        const int64_t T = a.T, K = a.K, H = a.H, Hkv = a.Hkv, d = a.d, N = (H + 2 * Hkv) * d;
        const size_t es = dtype == FL_DTYPE_BF16 ? 2 : 4, nx = (size_t)T * K, qbytes = (size_t)T * H * d * es;
        // the plan of the prompt path, as enqueue_forward asks for it
        const LinearPlan qp = form == 0 ? plan_qkv_rope(dtype, T, N, K, d, d * Hkv, B.L.tp, qkv_split(T)) : LinearPlan{};
        if (form == 0 && qp.rope && d != 64 && d != 128) FL_FAIL(FL_ERR_UNSUPPORTED, "fl_op_qkv_rope: form 0: the RoPE epilogue takes head_dim 64 / 128");
        if (a.kernels_out) {
            a.kernels_out[0] = form == 0 ? qp.kernel : (int)LK_GEMV; a.kernels_out[1] = form == 0 ? qp.ks : 1; a.kernels_out[2] = form == 0 && qp.n_main < N ? qp.tail : (int)LK_NONE;
            a.kernels_out[3] = form != 0 || qp.rope ? 1 : 0;
        }
        void *wd; float *sd = nullptr, *bd = nullptr, *ct, *sn, *nw;
        FL_TRY(B.upload(&wd, a.w, (size_t)N * K * (form == 2 ? 1 : es)));
        if (form == 2) FL_TRY(B.upload(&sd, a.w_scale, (size_t)N * 4));
        if (a.bias) FL_TRY(B.upload(&bd, a.bias, (size_t)N * 4));
        FL_TRY(B.upload(&ct, a.cos_tab, (size_t)a.max_pos * (d / 2) * 4));
        FL_TRY(B.upload(&sn, a.sin_tab, (size_t)a.max_pos * (d / 2) * 4));
        FL_TRY(B.upload(&nw, a.norm_w, (size_t)K * 4));
        // the norm's inputs, as fl_op_norm_linear holds them
        float *xr0 = nullptr, *xr = nullptr, *xo = nullptr, *dd = nullptr, *inv = nullptr, *yd = nullptr;
        void *xs = nullptr, *ed = nullptr, *qd; uint32_t *ids = nullptr;
        FL_TRY(B.alloc(&qd, qbytes));
        FL_TRY(B.alloc(&xo, nx * 4));
        if (a.delta) FL_TRY(B.upload(&dd, a.delta, nx * 4 * a.n_slab));
        if (a.embed) {
            FL_TRY(B.upload(&ed, a.embed, (size_t)a.vocab * K * es));
            FL_TRY(B.upload(&ids, a.tokens, (size_t)T * 4));
        } else {
            FL_TRY(B.upload(&xr0, a.x_res, nx * 4));
        }
        if (form == 0) {
            FL_TRY(B.alloc(&xs, nx * es));
            FL_TRY(B.alloc(&inv, (size_t)T * 4));
            if (!qp.rope) FL_TRY(B.alloc(&yd, (size_t)T * N * 4 * std::max(qp.n_split, 1)));
            xr = xo;                                                 // form 0 updates the residual rows in place: they are its x_out
        }
        RopeSeqsDev sq;
        FL_TRY(sq.upload(B, q, Hkv, d, es, a.embed ? a.tokens : nullptr));
        const int64_t sa = q.seq_alloc[0];
        const size_t kv_layer_off = (size_t)q.layer * Hkv * d, off0 = kv_layer_off * (size_t)sa * es;
        const bool vt0 = q.v_transposed[0] != 0;
        std::vector<unsigned char> first;
        FL_TRY(rope_op_repeat(B, "fl_op_qkv_rope", sq, qd, qbytes, xo, nx * 4, a.repeat, first, [&]() -> int {
            void *kl = (char *)sq.k[0] + off0, *vl = (char *)sq.v[0] + off0;
            if (form == 0) {
                if (a.embed) FL_TRY(launch_embed(B.L, dtype, ed, ids, nullptr, xr, T, K));
                else FL_HIP(hipMemcpyAsync(xr, xr0, nx * 4, hipMemcpyDeviceToDevice, B.s));
                FL_TRY(launch_rmsnorm_add(B.L, dtype, xr, dd, nw, a.eps, xs, inv, T, K, std::max(a.n_slab, 1), (int64_t)nx));
                if (qp.rope) {
                    RopeEpi ro;
                    ro.st = sq.st; ro.cos_tab = ct; ro.sin_tab = sn; ro.max_pos = (int)a.max_pos; ro.q_out = qd; ro.k_cache = kl; ro.v_cache = vl;
                    ro.H = (int)H; ro.Hkv = (int)Hkv; ro.d = (int)d; ro.max_seq = (int)sa; ro.v_transposed = vt0 ? 1 : 0;
                    return launch_plan(B.L, qp, dtype, wd, xs, bd, nullptr, T, N, K, EPI_QKV_ROPE, inv, nullptr, &ro);
                }
                FL_HIP(hipMemsetAsync(yd, 0xff, (size_t)T * N * 4 * std::max(qp.n_split, 1), B.s));
                FL_TRY(launch_plan(B.L, qp, dtype, wd, xs, nullptr, yd, T, N, K, EPI_F32, inv));
                return launch_rope_kv(B.L, dtype, yd, sq.st, ct, sn, a.max_pos, qd, kl, vl, T, H, Hkv, d, sa, vt0, qp.n_split, bd);
            }
            if (form == 3) {
                GemvBatchArgs ga;
                ga.B = (int)T; ga.seqs = sq.refs_dev; ga.W = wd; ga.bias = bd; ga.N = (int)N; ga.K = (int)K; ga.nks = 1;
                ga.epi = EPI_QKV_ROPE; ga.pro = PRO_NORM; ga.norm_w = nw; ga.eps = a.eps; ga.x_out = xo;
                if (a.embed) ga.embed = ed;
                else { ga.x_in = xr0; ga.delta = dd; ga.n_slab = std::max(a.n_slab, 1); ga.slab_stride = (long long)nx; }
                ga.cos_tab = ct; ga.sin_tab = sn; ga.q_out = qd; ga.kv_layer_off = kv_layer_off;
                ga.H = (int)H; ga.Hkv = (int)Hkv; ga.d = (int)d; ga.max_pos = (int)a.max_pos;
                return launch_gemv_batch(B.L, ga);
            }
            GemvArgs ga;                                             // as qkv_gemv_args (model.hip) lays it out
            ga.W = wd; ga.bias = bd; ga.N = (int)N; ga.K = (int)K; ga.epi = EPI_QKV_ROPE; ga.pro = PRO_NORM; ga.norm_w = nw; ga.eps = a.eps; ga.st = sq.st;
            ga.x_out = xo;
            if (a.embed) ga.embed = ed;
            else { ga.x_in = xr0; ga.delta = dd; ga.delta_nslab = std::max(a.n_slab, 1); }
            ga.cos_tab = ct; ga.sin_tab = sn; ga.q_out = qd; ga.k_cache = kl; ga.v_cache = vl;
            ga.H = (int)H; ga.Hkv = (int)Hkv; ga.d = (int)d; ga.max_seq = (int)sa; ga.max_pos = (int)a.max_pos; ga.v_ld = vt0 ? (int)sa : 0;
            return form == 1 ? launch_gemv(B.L, dtype, ga) : launch_gemv_w8(B.L, ga, sd);
        }));
        memcpy(a.q_out, first.data(), qbytes);
        if (a.x_out) memcpy(a.x_out, first.data() + qbytes, nx * 4);
        sq.give_back(q, first.data() + qbytes + nx * 4);
        return FL_OK;
    });
}

int fl_op_attn_oproj_rep(const fl_attn_oproj_rep_args *args) {
    return guarded([&]() -> int {
        AttnRepGeometry g;
        FL_TRY(attn_oproj_rep_check(args, &g));
        const fl_attn_oproj_rep_args &a = *args;
        const int info[6] = {g.model_rule ? 1 : 0, g.any_size ? 1 : 0, g.rpw, g.gmax, g.blocks, g.nslice};
        if (a.query_only) {
            memcpy(a.info_out, info, sizeof info);
            return FL_OK;
        }
        OpScope B;
        FL_TRY(B.begin());
        const int64_t H = a.H, Hkv = a.Hkv, d = a.d, N = a.N, K = H * d, sa = (a.capacity + 31) / 32 * 32;
        void *qd, *kd, *vd, *wd; float *od; StepState *std_;
        FL_TRY(B.upload(&qd, a.q, (size_t)K * 2));
        FL_TRY(B.upload(&wd, a.w_o, (size_t)N * K * 2));
        FL_TRY(B.alloc(&od, (size_t)a.repeat * N * 4));
        // the cache layout of the model: K [Hkv][sa][d], V transposed [Hkv][d][sa]
        FL_TRY(attn_op_upload_cache(B, &kd, &vd, FL_DTYPE_BF16, a.k, a.v, 1, a.k_rows, Hkv, sa, d, true, a.pad_value));
        StepState st{}; st.pos = (uint32_t)a.s_past; st.len = (uint32_t)a.s_past; st.call0 = (uint32_t)a.s_past; st.eos = -1;
        FL_TRY(B.upload(&std_, &st, sizeof st));
        AttnRepArgs ra;                                              // as the decode step of model.hip fills it, without the tensor-parallel epilogue
        ra.q = qd; ra.kc = kd; ra.vT = vd; ra.st = std_; ra.Wo = wd;
        ra.H = (int)H; ra.Hkv = (int)Hkv; ra.seq_alloc = (int)sa; ra.N = (int)N; ra.K = (int)K; ra.scale = 1.0f / sqrtf((float)d);
        for (int r = 0; r < a.repeat; r++) {
            ra.out = od + (size_t)r * N;
            FL_HIP(hipMemsetAsync(ra.out, 0xff, (size_t)N * 4, B.s));  // NaN pattern: a row the launch does not write shows up
            FL_TRY(launch_attn_oproj_rep(B.L, ra));
        }
        FL_HIP(hipStreamSynchronize(B.s));
        FL_HIP(hipMemcpy(a.out, od, (size_t)a.repeat * N * 4, hipMemcpyDeviceToHost));
        if (a.info_out) memcpy(a.info_out, info, sizeof info);
        return FL_OK;
    });
}

int fl_op_gemv_resid(const fl_gemv_resid_args *args) {
    return guarded([&]() -> int {
        if (!args) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_gemv_resid: null args");
        const fl_gemv_resid_args &a = *args;
        if (a.struct_size != sizeof(fl_gemv_resid_args)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_gemv_resid: struct_size %zu, expected %zu", a.struct_size, sizeof(fl_gemv_resid_args));
        if (a.mode < 0 || a.mode > 2 || a.epi2 < 0 || a.epi2 > 2) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_gemv_resid: mode 0..2, epi2 0..2");
        if (a.repeat < 1 || a.repeat > 8) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_gemv_resid: repeat %d not in 1..8", a.repeat);
        const bool prod = a.mode != 1, cons = a.mode != 0, pair = a.mode == 2;
        const int64_t N = a.N, K = a.K, N2 = a.N2, H = a.H, Hkv = a.Hkv, d = a.d, sa = a.seq_alloc;
        if (N <= 0 || N % 8 || N > (1 << 24)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_gemv_resid: N must be a multiple of 8");
        if (prod && (K <= 0 || K % 8 || !a.x || !a.w || !a.h_in || !a.w_next || !a.h_out || !a.xs_out || !a.cs_out || !a.delta_out))
            FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_gemv_resid: the producer takes x, w, h_in, w_next (K a multiple of 8) and gives h_out, xs_out, cs_out, delta_out");
        if (!prod && (!a.xs || !a.cs)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_gemv_resid: mode 1 takes xs and cs");
        if (cons) {
            if (!a.w2 || !a.y_out || !a.inv_out || N2 <= 0 || N2 > (1 << 24)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_gemv_resid: the consumer takes w2 [N2][N] and gives y_out, inv_out");
            if (a.epi2 == 1 && N2 % 2) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_gemv_resid: gate/up needs an even N2");
            if (a.epi2 == 2 && (H < 1 || Hkv < 1 || d < 2 || d % 2 || N2 != (H + 2 * Hkv) * d || a.max_pos < 1 || a.pos < 0 || a.pos >= a.max_pos || sa < 1 ||
                                sa > (1 << 20) || a.len < 0 || a.len >= sa || !a.cos_tab || !a.sin_tab))
                FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_gemv_resid: QKV: N2 = (H + 2 Hkv) d, pos < max_pos, len < seq_alloc, cos_tab / sin_tab");
            if (pair && (!a.h_ref || !a.y_ref || !a.inv_ref)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_gemv_resid: mode 2 gives h_ref, y_ref, inv_ref");
        }
        OpScope B;
        FL_TRY(B.begin());
        const int dt = FL_DTYPE_BF16;
        void *xd = nullptr, *wd = nullptr, *xsd, *w2d = nullptr; float *h0 = nullptr, *wn = nullptr, *h, *csd, *dl, *ct = nullptr, *sn = nullptr;
        StepState *std_ = nullptr;
        if (prod) {
            FL_TRY(B.upload(&xd, a.x, (size_t)K * 2)); FL_TRY(B.upload(&wd, a.w, (size_t)N * K * 2));
            FL_TRY(B.upload(&h0, a.h_in, (size_t)N * 4)); FL_TRY(B.upload(&wn, a.w_next, (size_t)N * 4));
        }
        FL_TRY(B.alloc(&h, (size_t)N * 4)); FL_TRY(B.alloc(&dl, (size_t)N * 4));
        FL_TRY(B.alloc(&xsd, (size_t)N * 2)); FL_TRY(B.alloc(&csd, (size_t)N / 8 * 4));
        // the consumer's matrix in its device layout, and one set of outputs per form: y (fp32 | packed silu(g)*u | q + one layer's
        // caches, V transposed as the MFMA attention keeps it), the ArgMax candidates
        int64_t N2w = N2, I2p = 0;
        const int cepi = a.epi2 == 1 ? EPI_GATEUP : a.epi2 == 2 ? EPI_QKV_ROPE : EPI_F32;
        struct ConsOut { void *y = nullptr, *k = nullptr, *v = nullptr; ArgmaxCand *amax = nullptr; float *h = nullptr, *dl = nullptr; };
        ConsOut co[2];
        const size_t ybytes = !cons ? 0 : a.epi2 == 1 ? (size_t)((N2 / 2 + 15) / 16 * 16) * 2 : a.epi2 == 2 ? (size_t)H * d * 2 : (size_t)N2 * 4;
        const size_t cbytes = cons && a.epi2 == 2 ? (size_t)Hkv * sa * d * 2 : 0;
        if (cons) {
            FL_TRY(op_upload_matrix(B, dt, a.w2, N2, N, cepi, &w2d, &N2w, &I2p));
            if (a.epi2 == 2) {
                FL_TRY(B.upload(&ct, a.cos_tab, (size_t)a.max_pos * (d / 2) * 4)); FL_TRY(B.upload(&sn, a.sin_tab, (size_t)a.max_pos * (d / 2) * 4));
            }
            StepState st{}; st.pos = (uint32_t)a.pos; st.len = (uint32_t)a.len; st.call0 = (uint32_t)a.len; st.eos = -1;
            FL_TRY(B.upload(&std_, &st, sizeof st));
            for (int f = 0; f < (pair ? 2 : 1); f++) {
                FL_TRY(B.alloc(&co[f].y, ybytes));
                if (cbytes) { FL_TRY(B.alloc(&co[f].k, cbytes)); FL_TRY(B.alloc(&co[f].v, cbytes)); }
                if (a.epi2 == 0) FL_TRY(B.alloc(&co[f].amax, sizeof(ArgmaxCand) * kMaxArgmaxCand));
                if (f) { FL_TRY(B.alloc(&co[f].h, (size_t)N * 4)); FL_TRY(B.alloc(&co[f].dl, (size_t)N * 4)); }
            }
        }
        auto consumer_args = [&](const ConsOut &o) {
            GemvArgs g;
            g.W = w2d; g.out = o.y; g.N = (int)N2w; g.K = (int)N; g.epi = cepi; g.eps = a.eps; g.st = std_;
            if (a.epi2 == 0 && gemv_leaves_candidates(dt, g)) g.amax = o.amax;
            if (a.epi2 == 2) {
                g.cos_tab = ct; g.sin_tab = sn; g.q_out = o.y; g.k_cache = o.k; g.v_cache = o.v; g.out = nullptr;
                g.H = (int)H; g.Hkv = (int)Hkv; g.d = (int)d; g.max_seq = (int)sa; g.max_pos = (int)a.max_pos; g.v_ld = (int)sa;
            }
            return g;
        };
        auto clear = [&](const ConsOut &o) -> int {              // NaN patterns: what no launch writes shows up
            FL_HIP(hipMemsetAsync(o.y, 0xff, ybytes, B.s));
            if (cbytes) { FL_HIP(hipMemsetAsync(o.k, 0xff, cbytes, B.s)); FL_HIP(hipMemsetAsync(o.v, 0xff, cbytes, B.s)); }
            if (o.amax) FL_HIP(hipMemsetAsync(o.amax, 0xff, sizeof(ArgmaxCand) * kMaxArgmaxCand, B.s));
            return FL_OK;
        };
        // the bytes one run left: h | delta | xs | cs, then per form y | k | v | candidates (and the old form's h | delta)
        const size_t abytes = a.epi2 == 0 && cons ? sizeof(ArgmaxCand) * kMaxArgmaxCand : 0;
        const size_t off_dl = (size_t)N * 4, off_xs = off_dl + (size_t)N * 4, off_cs = off_xs + (size_t)N * 2, off_c = off_cs + (size_t)N / 8 * 4;
        const size_t per = ybytes + 2 * cbytes + abytes + (size_t)N * 8, total = off_c + 2 * per;
        std::vector<unsigned char> first(total, 0), again(total, 0);
        for (int rep = 0; rep < a.repeat; rep++) {
            FL_HIP(hipMemsetAsync(h, 0xff, (size_t)N * 4, B.s)); FL_HIP(hipMemsetAsync(dl, 0xff, (size_t)N * 4, B.s));
            if (prod) {
                FL_HIP(hipMemsetAsync(xsd, 0xff, (size_t)N * 2, B.s)); FL_HIP(hipMemsetAsync(csd, 0xff, (size_t)N / 8 * 4, B.s));
                GemvArgs p;                                          // as the step builder's producer (model.hip) lays it out
                p.W = wd; p.x = xd; p.out = dl; p.N = (int)N; p.K = (int)K; p.epi = EPI_RESID; p.pro = PRO_X;
                p.x_in = h0; p.norm_w = wn; p.x_out = h; p.xs_out = xsd; p.cs_out = csd;
                FL_TRY(launch_gemv(B.L, dt, p));
            } else {
                FL_HIP(hipMemcpyAsync(xsd, a.xs, (size_t)N * 2, hipMemcpyHostToDevice, B.s)); FL_HIP(hipMemcpyAsync(csd, a.cs, (size_t)N / 8 * 4, hipMemcpyHostToDevice, B.s));
            }
            if (cons) {
                FL_TRY(clear(co[0]));
                GemvArgs g = consumer_args(co[0]);
                g.pro = PRO_XS; g.x = xsd; g.cs = csd;
                FL_TRY(launch_gemv(B.L, dt, g));
            }
            if (pair) {                                              // the same inputs through today's two launches
                FL_TRY(clear(co[1]));
                FL_HIP(hipMemsetAsync(co[1].h, 0xff, (size_t)N * 4, B.s)); FL_HIP(hipMemsetAsync(co[1].dl, 0xff, (size_t)N * 4, B.s));
                GemvArgs p;
                p.W = wd; p.x = xd; p.out = co[1].dl; p.N = (int)N; p.K = (int)K; p.epi = EPI_F32; p.pro = PRO_X;
                FL_TRY(launch_gemv(B.L, dt, p));
                GemvArgs g = consumer_args(co[1]);
                g.pro = PRO_NORM; g.x_in = h0; g.delta = co[1].dl; g.norm_w = wn; g.x_out = co[1].h;
                FL_TRY(launch_gemv(B.L, dt, g));
            }
            FL_HIP(hipStreamSynchronize(B.s));
            unsigned char *o = (rep ? again : first).data();
            FL_HIP(hipMemcpy(o, h, (size_t)N * 4, hipMemcpyDeviceToHost)); FL_HIP(hipMemcpy(o + off_dl, dl, (size_t)N * 4, hipMemcpyDeviceToHost));
            FL_HIP(hipMemcpy(o + off_xs, xsd, (size_t)N * 2, hipMemcpyDeviceToHost)); FL_HIP(hipMemcpy(o + off_cs, csd, (size_t)N / 8 * 4, hipMemcpyDeviceToHost));
            for (int f = 0; cons && f < (pair ? 2 : 1); f++) {
                unsigned char *c = o + off_c + (size_t)f * per;
                FL_HIP(hipMemcpy(c, co[f].y, ybytes, hipMemcpyDeviceToHost)); c += ybytes;
                if (cbytes) { FL_HIP(hipMemcpy(c, co[f].k, cbytes, hipMemcpyDeviceToHost)); FL_HIP(hipMemcpy(c + cbytes, co[f].v, cbytes, hipMemcpyDeviceToHost)); }
                c += 2 * cbytes;
                if (co[f].amax) FL_HIP(hipMemcpy(c, co[f].amax, abytes, hipMemcpyDeviceToHost));
                c += abytes;
                if (f) { FL_HIP(hipMemcpy(c, co[f].h, (size_t)N * 4, hipMemcpyDeviceToHost)); FL_HIP(hipMemcpy(c + (size_t)N * 4, co[f].dl, (size_t)N * 4, hipMemcpyDeviceToHost)); }
            }
            if (rep && first != again) FL_FAIL(FL_ERR_HIP, "fl_op_gemv_resid: launch %d gave other bytes than the first", rep);
        }
        // 1/m as each prologue computes it, read through a probe launch on the sums the run left: the staged vector is 1.0 at one
        // element j and +-0 elsewhere, the matrix (the consumer's shape, fp32 epilogue) is 1.0 at [0][j], so row 0 comes out as 1.0 * 1/m.
        // PRO_XS stages such a vector next to the producer's cs; PRO_NORM is given the norm weight 1 / v[j] at j (v[j] * w rounds to
        // bf16 1.0 whatever its last fp32 bits are) and 0 elsewhere, next to the x_in and delta of the run.
        if (cons) {
            const float *hv = reinterpret_cast<const float *>(first.data() + off_c + per + ybytes + 2 * cbytes + abytes);
            int64_t j = 0;
            float wj = 1.0f;
            if (pair) {
                for (j = 0; j < N; j++)
                    if (std::isfinite(hv[j]) && fabsf(hv[j]) >= 1e-3f && fabsf(hv[j]) <= 1e3f) break;
                if (j == N) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_gemv_resid: no element of h between 1e-3 and 1e3 to probe 1/m with");
                wj = 1.0f / hv[j];
            }
            std::vector<bf16_t> xp((size_t)N, 0);
            std::vector<float> wp((size_t)N, 0.f);
            xp[(size_t)j] = 0x3f80; wp[(size_t)j] = wj;
            void *xpd, *Wp; float *wpd, *yp;
            FL_TRY(B.upload(&xpd, xp.data(), (size_t)N * 2)); FL_TRY(B.upload(&wpd, wp.data(), (size_t)N * 4));
            FL_TRY(B.alloc(&Wp, (size_t)N2w * N * 2)); FL_TRY(B.alloc(&yp, (size_t)N2w * 4));
            FL_HIP(hipMemsetAsync(Wp, 0, (size_t)N2w * N * 2, B.s));
            FL_HIP(hipMemcpyAsync((bf16_t *)Wp + j, &xp[(size_t)j], 2, hipMemcpyHostToDevice, B.s));
            for (int f = 0; f < (pair ? 2 : 1); f++) {
                FL_HIP(hipMemsetAsync(yp, 0xff, (size_t)N2w * 4, B.s));
                GemvArgs g;
                g.W = Wp; g.out = yp; g.N = (int)N2w; g.K = (int)N; g.epi = EPI_F32; g.eps = a.eps; g.st = std_;
                if (f) { g.pro = PRO_NORM; g.x_in = h0; g.delta = co[1].dl; g.norm_w = wpd; }
                else { g.pro = PRO_XS; g.x = xpd; g.cs = csd; }
                FL_TRY(launch_gemv(B.L, dt, g));
                FL_HIP(hipStreamSynchronize(B.s));
                FL_HIP(hipMemcpy(f ? a.inv_ref : a.inv_out, yp, 4, hipMemcpyDeviceToHost));
            }
        }
        if (prod) {
            memcpy(a.h_out, first.data(), (size_t)N * 4); memcpy(a.delta_out, first.data() + off_dl, (size_t)N * 4);
            memcpy(a.xs_out, first.data() + off_xs, (size_t)N * 2); memcpy(a.cs_out, first.data() + off_cs, (size_t)N / 8 * 4);
        }
        for (int f = 0; cons && f < (pair ? 2 : 1); f++) {
            const unsigned char *c = first.data() + off_c + (size_t)f * per;
            float *y = f ? a.y_ref : a.y_out;
            const bf16_t *yb = reinterpret_cast<const bf16_t *>(c);
            if (a.epi2 == 0) {
                memcpy(y, c, ybytes);
            } else if (a.epi2 == 1) {
                for (int64_t j = 0; j < N2 / 2; j++) y[j] = bf16_bits_to_float(yb[j]);
            } else {                                                 // q | the appended k row | the appended v row
                const bf16_t *kb = reinterpret_cast<const bf16_t *>(c + ybytes), *vb = reinterpret_cast<const bf16_t *>(c + ybytes + cbytes);
                for (int64_t j = 0; j < H * d; j++) y[j] = bf16_bits_to_float(yb[j]);
                for (int64_t hd = 0; hd < Hkv; hd++)
                    for (int64_t j = 0; j < d; j++) {
                        y[H * d + hd * d + j] = bf16_bits_to_float(kb[(hd * sa + a.len) * d + j]);
                        y[(H + Hkv) * d + hd * d + j] = bf16_bits_to_float(vb[(hd * d + j) * sa + a.len]);
                    }
            }
            c += ybytes + 2 * cbytes;
            if (a.amax_out) {                                        // the row the candidates give (ties: the larger index), -1 without candidates
                int best = -1;
                if (abytes) {
                    const ArgmaxCand *cand = reinterpret_cast<const ArgmaxCand *>(c);
                    float bv = 0.f;
                    const int n = cand[0].i;
                    for (int i = 1; n > 0 && n < kMaxArgmaxCand && i <= n; i++)
                        if (cand[i].i >= 0 && (best < 0 || cand[i].v > bv || (cand[i].v == bv && cand[i].i > best))) { bv = cand[i].v; best = cand[i].i; }
                }
                a.amax_out[f] = best;
            }
            c += abytes;
            if (f) memcpy(a.h_ref, c, (size_t)N * 4);
        }
        return FL_OK;
    });
}

int fl_op_convert_slice(const fl_convert_slice_args *args) {
    return guarded([&]() -> int {
        FL_TRY(convert_slice_check(args));
        const fl_convert_slice_args &a = *args;
        OpScope B;
        FL_TRY(B.begin());
        const size_t ses = a.src_dtype == FL_DTYPE_F32 ? 4 : 2, des = a.dst_dtype == FL_DTYPE_F32 ? 4 : 2;
        const size_t dbytes = (size_t)a.dst_rows * a.dst_ld * des;
        void *sd, *dd;
        FL_TRY(B.upload(&sd, a.src, (size_t)a.R * a.C * ses));
        FL_TRY(B.alloc(&dd, dbytes));
        FL_HIP(hipMemsetAsync(dd, 0xff, dbytes, B.s));             // NaN pattern: an element the launch leaves alone shows up
        FL_TRY(launch_convert_slice(B.L, a.src_dtype, sd, a.C, a.r0, a.c0, a.rows, a.cols, a.dst_dtype, dd, a.dst_ld, a.dst_row0, a.row_mode,
                                    a.head_pad, a.head_pad ? a.dm : 0, a.head_pad ? a.d : 0, a.via_bf16));
        FL_HIP(hipStreamSynchronize(B.s));
        FL_HIP(hipMemcpy(a.dst, dd, dbytes, hipMemcpyDeviceToHost));
        return FL_OK;
    });
}

int fl_op_model_tensor(fl_model *m, int32_t shard, int32_t selector, int64_t layer, void *out, int64_t *rows_out, int64_t *cols_out,
                       int32_t *elem_out) {
    return guarded([&]() -> int {
        if (!m || !rows_out || !cols_out || !elem_out) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_model_tensor: null argument (model, rows_out, cols_out, elem_out)");
        Model *mm = M(m);
        std::lock_guard<std::mutex> lock(mm->mu);
        if (shard < 0 || (size_t)shard >= mm->shards.size()) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_model_tensor: shard %d not below %zu local shards", shard, mm->shards.size());
        if (selector < FL_MT_EMBED || selector > FL_MT_LM_HEAD_S) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_model_tensor: unknown selector %d", selector);
        const bool per_layer = (selector >= FL_MT_WQKV && selector <= FL_MT_LN2) || (selector >= FL_MT_WQKV_Q && selector <= FL_MT_WD_S);
        if (per_layer && (layer < 0 || layer >= mm->D.L)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_model_tensor: layer %lld not below %lld", (long long)layer, (long long)mm->D.L);
        const Dims &D = mm->D;
        Shard &sh = mm->shards[(size_t)shard];
        const LayerW none, &ly = per_layer ? sh.layers[(size_t)layer] : none;
        const int64_t nq = (sh.Hs + 2 * sh.Hkvs) * D.d, half = D.d / 2;
        const int wdt = mm->dtype;
        const void *p = nullptr; int64_t R = 0, C = 0; int elem = FL_DTYPE_F32;
        auto is = [&](const void *ptr, int64_t r, int64_t c, int e) { p = ptr; R = r; C = c; elem = e; };
        switch (selector) {
            case FL_MT_EMBED:     is(sh.embed, D.V, D.h, wdt); break;
            case FL_MT_NORM:      is(sh.norm, D.h, 1, FL_DTYPE_F32); break;
            case FL_MT_LM_HEAD:   is(sh.lm_head, sh.Vs, D.h, wdt); break;
            case FL_MT_COS_TAB:   is(sh.cos_tab, D.max_pos, half, FL_DTYPE_F32); break;
            case FL_MT_SIN_TAB:   is(sh.sin_tab, D.max_pos, half, FL_DTYPE_F32); break;
            case FL_MT_WQKV:      is(ly.wqkv, nq, D.h, wdt); break;
            case FL_MT_BQKV:      is(ly.bqkv, nq, 1, FL_DTYPE_F32); break;
            case FL_MT_WO:        is(ly.wo, D.h, sh.Hs * D.d, wdt); break;
            case FL_MT_WGU:       is(ly.wgu, 2 * sh.Ip, D.h, wdt); break;
            case FL_MT_WD:        is(ly.wd, D.h, sh.Ip, wdt); break;
            case FL_MT_LN1:       is(ly.ln1, D.h, 1, FL_DTYPE_F32); break;
            case FL_MT_LN2:       is(ly.ln2, D.h, 1, FL_DTYPE_F32); break;
            case FL_MT_WQKV_Q:    is(ly.wqkv8, nq, D.h, FL_ELEM_E4M3); break;
            case FL_MT_WQKV_S:    is(ly.sqkv, nq, 1, FL_DTYPE_F32); break;
            case FL_MT_WO_Q:      is(ly.wo8, D.h, sh.Hs * D.d, FL_ELEM_E4M3); break;
            case FL_MT_WO_S:      is(ly.so, D.h, 1, FL_DTYPE_F32); break;
            case FL_MT_WGU_Q:     is(ly.wgu8, 2 * sh.Ip, D.h, FL_ELEM_E4M3); break;
            case FL_MT_WGU_S:     is(ly.sgu, 2 * sh.Ip, 1, FL_DTYPE_F32); break;
            case FL_MT_WD_Q:      is(ly.wd8, D.h, sh.Ip, FL_ELEM_E4M3); break;
            case FL_MT_WD_S:      is(ly.sd, D.h, 1, FL_DTYPE_F32); break;
            case FL_MT_LM_HEAD_Q: is(sh.lm_head8, sh.Vs, D.h, FL_ELEM_E4M3); break;
            default:              is(sh.lm_head_s, sh.Vs, 1, FL_DTYPE_F32); break;      // FL_MT_LM_HEAD_S
        }
        if (!p) FL_FAIL(FL_ERR_BAD_ARGUMENT, "fl_op_model_tensor: this model has no tensor for selector %d (q/k/v bias, FL_WEIGHTS_E4M3_ROW)", selector);
        *rows_out = R; *cols_out = C; *elem_out = elem;
        if (!out) return FL_OK;
        const size_t es = elem == FL_DTYPE_F32 ? 4 : (elem == FL_ELEM_E4M3 ? 1 : 2);
        FL_HIP(hipSetDevice(sh.device));
        FL_HIP(hipStreamSynchronize(sh.stream));
        FL_HIP(hipMemcpy(out, p, (size_t)R * C * es, hipMemcpyDeviceToHost));
        return FL_OK;
    });
}

}  // extern "C"
