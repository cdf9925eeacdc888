// kernels.h -- host-callable launch wrappers of the gfx950 kernels.
#pragma once
#include <vector>

#include "common.h"

namespace fl {

// Kernel classes for the measurement hooks (fl_profile_*): one class per kernel symbol family.
enum KernelClass {
    KC_EMBED = 0, KC_RMSNORM, KC_GEMV, KC_GEMM_MFMA, KC_GEMM_GENERIC, KC_ROPE_KV, KC_ATTN_DECODE,
    KC_ATTN_COMBINE, KC_ATTN_PREFILL, KC_ARGMAX, KC_REDUCE, KC_CONVERT, KC_ATTN_OPROJ, KC_COMM, KC_KVCOPY,
    KC_ENC_EMBED_LN, KC_ENC_ADD_LN, KC_ENC_BIAS_ACT, KC_ENC_ATTN, KC_ENC_POOL, KC_COUNT
};
const char *kernel_class_name(int kc);

struct ProfRecord { int kc; double bytes, flops; hipEvent_t e0, e1; char tag[32]; };

// 1/rms of the rows a residual epilogue (EPI_RESID) left, taken by the CONSUMING projection itself from the partial sums of squares
// -- row t: 1 / sqrt(sum_i part[t][i] / h + eps), summed left to right -- instead of an rms_finalize launch in between.  Honoured by
// the 256 x 256 kernels' plain launches and by the 128 x 256 kernel (LinearPlan::reads_rs_parts tells); everything else ignores it.
struct RsParts { const float *part = nullptr; int np = 0; float eps = 0.f, inv_h = 0.f; };

// Launch context: the stream a kernel goes to and, while profiling, where its event pair is kept.
struct Launcher {
    hipStream_t stream = nullptr;
    RsParts rsp;                               // non-null part: the next projection's row scales come from these partial sums
    std::vector<ProfRecord> *prof = nullptr;   // non-null: bracket every launch with HIP events
    const char *tag = "";                      // optional sub-class label for the profile (shape, variant)
    int tp = 1;                                // tensor-parallel degree of the model this launch belongs to (> 1: a rank's shard shapes -- launch_linear plans for those)

    template <typename... KArgs, typename... Args>
    int launch(int kc, double bytes, double flops, void (*kernel)(KArgs...), dim3 grid, dim3 block,
               size_t lds, Args... args) {
        if (grid.x == 0 || grid.y == 0 || grid.z == 0) return FL_OK;
        if (prof) {
            ProfRecord r{kc, bytes, flops, nullptr, nullptr, {0}};
            snprintf(r.tag, sizeof r.tag, "%s", tag ? tag : "");
            FL_HIP(hipEventCreate(&r.e0));
            FL_HIP(hipEventCreate(&r.e1));
            hipExtLaunchKernelGGL(kernel, grid, block, (uint32_t)lds, stream, r.e0, r.e1, 0, static_cast<KArgs>(args)...);
            prof->push_back(r);
        } else {
            hipLaunchKernelGGL(kernel, grid, block, (uint32_t)lds, stream, static_cast<KArgs>(args)...);
        }
        FL_HIP(hipGetLastError());
        return FL_OK;
    }
};

int device_cu_count();   // CUs of the current device, cached per device (runtime.hip); 256 where the runtime does not tell

enum { EPI_F32 = 0, EPI_GATEUP = 1, EPI_QKV_ROPE = 2, EPI_RESID = 3 };
// EPI_RESID (prefill GEMMs; the decode stream's form: GemvArgs below): the o_proj / down_proj epilogue takes over the residual add and the next
// RMSNorm's first pass -- h += y (fp32, in place), xn = (h + y) * w in the compute dtype, and partial sums of squares of
// h + y per (row, column tile, wave column) that rms_finalize turns into 1/rms -- instead of a y round trip through
// HBM and an rmsnorm_add launch.
struct ResidEpi {
    float *h = nullptr;            // [T][N] residual stream
    const float *w = nullptr;      // [N] weight of the NEXT RMSNorm
    void *xn = nullptr;            // [T][N] bf16
    float *part = nullptr;         // [T][np]
    int np = 0;
};
enum { PRO_X = 0, PRO_NORM = 1, PRO_XS = 2 };   // PRO_XS (decode stream): the normalised vector and its chunk sums of squares, left by an EPI_RESID launch

struct LLTable;
// Arguments of the decode weight-streaming kernel (k_gemv.hip), passed by value as kernarg.
struct ArgmaxCand { float v; int i; };   // [0]: {unused, count}; [1 + workgroup]: its best row
constexpr int kMaxArgmaxCand = 1024;

struct GemvArgs {
    const void *W = nullptr;        // [N,K] compute dtype
    const void *x = nullptr;        // PRO_X: [K] compute dtype
    const float *x_scale = nullptr; // PRO_X: optional scalar applied to the accumulator (1/rms)
    const float *bias = nullptr;    // [N] or null
    void *out = nullptr;            // EPI_F32: float[N]; EPI_GATEUP: XT[N/2]
    int N = 0, K = 0, epi = EPI_F32, pro = PRO_X;
    // PRO_NORM: x = rmsnorm(x_in + delta) * norm_w, or of the embedding row of st->token
    const float *x_in = nullptr, *delta = nullptr, *norm_w = nullptr;
    int delta_nslab = 1;            // delta is this many [K] vectors, K floats apart, added to x_in one by one in order (the fused attention + o_proj launch leaves one per kv head)
    float eps = 0.f;
    float *x_out = nullptr;         // updated residual, written by workgroup 0 (must differ from x_in)
    const void *embed = nullptr;    // [V,K] compute dtype, or null
    const StepState *st = nullptr;
    // EPI_QKV_ROPE: rows are q | k | v heads of width d; RoPE + KV append fused
    const float *cos_tab = nullptr, *sin_tab = nullptr;
    void *q_out = nullptr, *k_cache = nullptr, *v_cache = nullptr;
    int H = 0, Hkv = 0, d = 0, max_seq = 0, max_pos = 0;
    int v_ld = 0;                   // > 0: value cache is transposed [Hkv][d][v_ld] (MFMA attention layout)
    // EPI_F32 of a row-parallel projection in a tensor-parallel group: out = sum over ranks, exchanged in the epilogue
    const LLTable *ll = nullptr;    // device-resident; null = plain local output
    int ll_slot = 0;                // 1 .. LLTable::slots: which all-reduce of the decode step this is
    // EPI_F32 (the lm_head launch of a decode step): every workgroup also leaves the ArgMax of the rows it computed
    // ((value, index) pairs; ties -> the larger index, as argmax_last), so that token selection reads gridDim.x candidates
    // instead of the whole vocabulary; amax[0] is the candidate count.  null = not wanted.
    ArgmaxCand *amax = nullptr;
    // EPI_RESID (bf16, PRO_X, no bias / ll; the o_proj / down_proj of a decode step where gemv_resid_edge_fits): v = x_in + W . x goes
    // to x_out, bf16(v * norm_w) to xs_out [N] and the sum of squares of every 8 consecutive v to cs_out [N / 8]; `out` is not written.
    // Its grid must cover N exactly with one row group per wave: FL_ERR_UNSUPPORTED otherwise.
    void *xs_out = nullptr;
    float *cs_out = nullptr;
    // PRO_XS (bf16): x = such an xs [K], cs = such a cs [K / 8]: the RMSNorm of PRO_NORM with the residual add, v * w and the squares
    // already done; one chunk per staging thread (FL_ERR_UNSUPPORTED where the grid's workgroups have fewer than K / 8 threads)
    const float *cs = nullptr;
};
int launch_gemv(Launcher &L, int dtype, const GemvArgs &a);
// bytes of W that workgroup b of the plain-epilogue launch (no norm prologue) of an N x K matrix reads as one contiguous piece
// ([b chunk, (b + 1) chunk), then every grid-th piece): what a prefetcher needs to know to warm the right XCD's L2
int64_t gemv_owner_chunk(int dtype, int64_t N, int64_t K);
bool gemv_leaves_candidates(int dtype, const GemvArgs &a);   // the grid launch_gemv would pick fits the candidate buffer
bool gemv_norm_supported(int dtype, int64_t N, int64_t K);
// gemv_resid_edge (gemv_geometry.h) for an [N, K] producer and an [Nc, N] consumer on the current device, under the fl_tune grid and "gemv_r"
bool gemv_resid_edge_fits(int dtype, bool one_shard, bool compute_weights, int64_t N, int64_t K, int64_t Nc);
void gemv_set_tuning(int blocks, int waves);   // fl_tune "gemv_blocks" / "gemv_waves": force the grid / waves per workgroup (0 automatic, -1 keep)

// ---- FP8 weights (k_gemv_w8.hip): W' = s[row] * q, q e4m3fn, s a power of two per row (FL_WEIGHTS_E4M3_ROW) ------------
// the decode stream over them: GemvArgs as for launch_gemv with W = the e4m3 bytes [N,K], x / caches / out bf16 model types;
// no fused all-reduce (ll) and no sliced delta
int launch_gemv_w8(Launcher &L, const GemvArgs &a, const float *wscale /* [N] */);
bool gemv_w8_supported(int64_t N, int64_t K);          // K a multiple of 16 (a lane's 16-byte load)
bool gemv_w8_norm_supported(int64_t N, int64_t K);
bool gemv_w8_leaves_candidates(int64_t N, int64_t K);  // its grid fits the ArgMax candidate buffer
// src [N,K] bf16 / fp32 -> q [N,K], s [N] and (img non-null; may be src when that is bf16) the bf16 image s * q
int launch_quantize_rows(Launcher &L, int src_dtype, const void *src, int64_t N, int64_t K, uint8_t *q, float *s, void *img_bf16);
// rows in HF order (gate [0, I) | up [I, 2 I)) -> the 16-interleaved decode layout (test hook)
int launch_w8_gateup_layout(Launcher &L, const uint8_t *q, const float *s, int64_t I, int64_t K, uint8_t *qo, float *so);

// k_kvcopy.hip: a 2-D byte copy on the device, `rows` rows of `width` bytes (a multiple of 2) with a source and a destination pitch
// (multiples of 16, >= width; 16-byte aligned bases).  launch_kv_copy moves two such jobs -- the K and the V prefix of a cache -- in
// ONE launch and writes exactly the bytes [0, width) of every destination row.  kv_copy_check (the shape alone, no pointers): FL_ERR_BAD_ARGUMENT for anything else.
struct KvCopyJob { const void *src = nullptr; void *dst = nullptr; int64_t rows = 0, width = 0, spitch = 0, dpitch = 0; };
int kv_copy_check(const KvCopyJob &j);
int launch_kv_copy(Launcher &L, const KvCopyJob &a, const KvCopyJob &b);

// ---- the persistent decode engine (k_engine.hip): a chain of projections in one launch ---------------------------
constexpr int ENG_GATHER_WAVES = 4, ENG_STREAM_WAVES = 8, ENG_MAX_OPS = 4;
enum { ENG_IN_X = 0, ENG_IN_NORM = 1, ENG_IN_ACT = 2 };                 // plain bf16 vector of the previous launch | fp32 delta edge + residual + RMSNorm weight | packed silu(g)*u edge
enum { ENG_OUT_EDGE_F32 = 0, ENG_OUT_EDGE_ACT = 1, ENG_OUT_QKV = 2, ENG_OUT_LOGITS = 3 };
struct EngOp {
    const void *W = nullptr;            // [N,K] bf16
    int N = 0, K = 0, in = ENG_IN_X, out = ENG_OUT_EDGE_F32;
    int R = 2;                          // rows per wave item (launch_engine: 1 for row-parallel ops with few rows per CU)
    const void *x = nullptr;            // ENG_IN_X: bf16 [K]
    const float *norm_w = nullptr;      // ENG_IN_NORM: weight of the RMSNorm in front of this op
    const unsigned long long *in_edge = nullptr;   // granules {value, tag} written by the previous op of this launch
    unsigned long long *out_edge = nullptr;
    float *res_out = nullptr;           // ENG_IN_NORM: workgroup 0 also leaves the updated residual stream here (the next launch's x_res_in)
    void *dst = nullptr;                // ENG_OUT_LOGITS: float [N]
    const float *bias = nullptr;        // ENG_OUT_QKV / ENG_OUT_LOGITS
    int tag_in = 0, tag_out = 0;        // 1..255, unique per (launch of the step, edge)
};
struct EngArgs {
    EngOp op[ENG_MAX_OPS];
    int nops = 0, h = 0;
    const float *x_res_in = nullptr;    // [h] residual stream in front of the first op's layer (null: no op of the chain norms)
    float eps = 0.f;
    const StepState *st = nullptr;
    StepState *st_rw = nullptr;         // error word of a wait that gave up
    const uint32_t *epoch = nullptr;    // device word advanced once per decode step (select_advance): tags never repeat
    long long timeout_ticks = 0;        // wall_clock64 ticks (100 MHz)
    // ENG_OUT_QKV: RoPE + KV append as in GemvArgs
    const float *cos_tab = nullptr, *sin_tab = nullptr;
    void *q_out = nullptr, *k_cache = nullptr, *v_cache = nullptr;
    int H = 0, Hkv = 0, d = 0, max_seq = 0, max_pos = 0, v_ld = 0;
    ArgmaxCand *amax = nullptr;         // ENG_OUT_LOGITS: one ArgMax candidate per workgroup (as GemvArgs::amax)
    unsigned long long *stamps = nullptr;   // diagnostics: [workgroup][32] wall_clock64 stamps (FL_ENGINE_STAMPS)
    int grid = 0;                       // 0: one workgroup per CU
    int xs0_bytes = 0, xs1_bytes = 0;   // (filled by launch_engine)
    int pf_blocks = 1;                  // 8-KiB blocks a streamer requests ahead of an op's input (FL_ENGINE_PF)
    int gather_delay = 0;               // s_sleep(1) rounds between "this CU's streamers are done" and the first sweep (FL_ENGINE_DELAY)
};
bool engine_shape_ok(int64_t h, int64_t Hd, int64_t I, int64_t N_last);
int launch_engine(Launcher &L, const EngArgs &a);
void engine_set_grid(int workgroups);   // fl_tune("engine_grid"): 0 = one per CU

// ---- batched decode (k_gemv_batch.hip): B <= 8 sequences share one read of the weights ------------
// Per-sequence device state and buffers of a batch member (a view of its cache).
struct SeqRef {
    StepState *st;
    SampleState *ss;
    void *k, *v;                    // cache bases [L][Hkv][seq_alloc][d] / V^T [L][Hkv][d][seq_alloc]
    float *part_m, *part_l, *part_o;
    unsigned *counters;
    uint32_t *out_tokens;
    float *sel_scratch;
    int seq_alloc, nsplit;
};
struct GemvBatchArgs {
    const void *W = nullptr;        // [N,K] bf16
    const float *bias = nullptr;
    void *out = nullptr;            // EPI_F32: float [nks][B][N]; EPI_GATEUP: bf16 [B][N/2]
    int N = 0, K = 0, epi = EPI_F32, pro = PRO_X, B = 1, nks = 1;
    const void *x = nullptr;        // PRO_X: bf16 [B][K]
    const float *x_scale = nullptr; // PRO_X (k_gemv_dma.hip): optional [B] factors applied to the accumulators (1/rms of a separate norm)
    // PRO_NORM: x[b] = rmsnorm(x_in[b] + sum_s delta[s][b]) * norm_w, or of the embedding row of seqs[b].st->token
    const float *x_in = nullptr, *delta = nullptr, *norm_w = nullptr;
    int delta_nslab = 1;            // delta is the sum of this many [K] vectors, K floats apart (the fused attention + o_proj launch leaves one per kv head)
    int n_slab = 1; long long slab_stride = 0;
    float eps = 0.f;
    float *x_out = nullptr;         // [B][K] updated residual (must differ from x_in)
    const void *embed = nullptr;
    const SeqRef *seqs = nullptr;   // device array [B]
    // EPI_QKV_ROPE
    const float *cos_tab = nullptr, *sin_tab = nullptr;
    void *q_out = nullptr;          // bf16 [B][H*d]
    size_t kv_layer_off = 0;        // layer * Hkv * d: multiplied by the sequence's seq_alloc inside
    int H = 0, Hkv = 0, d = 0, max_pos = 0;
};
int gemv_batch_ksplit(int B, int64_t K, int64_t N, int epi);
int launch_gemv_batch(Launcher &L, const GemvBatchArgs &a);
// the same projections with the weights streamed by LDS-DMA into wave-private rings (k_gemv_dma.hip; 3 <= B <= 32 rows: a batch's streams or a short prompt's tokens)
bool gemv_dma_supported(int B, int64_t N, int64_t K, int epi, int d);
int gemv_dma_ksplit(int64_t K, int64_t N, int epi);
int launch_gemv_dma(Launcher &L, const GemvBatchArgs &a);
// q / out bf16 [B][H*d]; kv_layer_off = layer * Hkv * d (times each sequence's seq_alloc inside)
int launch_attn_decode_mfma_batch(Launcher &L, const void *q, const SeqRef *seqs_dev, int B, int max_nsplit, size_t kv_layer_off,
                                  void *out, int64_t H, int64_t Hkv, int64_t d, float scale, double kv_bytes_hint);
int launch_embed_batch(Launcher &L, const void *E, const SeqRef *seqs_dev, float *x_res, int B, int64_t h, int dtype = FL_DTYPE_BF16);
// the plain-layout batch attention (k_attn.hip): fp32 models, bf16 caches outside the MFMA attention layout; head_dim 64 / 128
bool attn_decode_batch_supported(int64_t d);
int launch_attn_decode_batch(Launcher &L, int dtype, const void *q, const SeqRef *seqs_dev, int B, int max_nsplit, size_t kv_layer_off, void *out,
                             int64_t H, int64_t Hkv, int64_t d, float scale);
// n_slab: K slices of the QKV projection ([n_slab][B][(H+2Hkv)*d] fp32, summed here); bias: added here (a K-sliced
// projection cannot add it itself) or null
int launch_rope_kv_batch(Launcher &L, const float *qkv, const SeqRef *seqs_dev, const float *cos_tab, const float *sin_tab,
                         int64_t max_pos, void *q_out, size_t kv_layer_off, int B, int64_t H, int64_t Hkv, int64_t d, int n_slab = 1,
                         const float *bias = nullptr, int dtype = FL_DTYPE_BF16, bool v_transposed = true);
// logits fp32 [B][V] -> every sequence's token / step state
int launch_unshard_logits(Launcher &L, const float *in, float *out, int tp, int B, int64_t Vs);   // [tp][B][Vs] -> [B][tp * Vs]
int launch_select_advance_batch(Launcher &L, const float *logits, int64_t V, const SeqRef *seqs_dev, int B, int advance);

// ---- packed prefill (k_prefill_packed.hip): several prompts' tokens back to back in one [T_total][..] forward -------------------------
// The device table of one call, built by the host: who a row is, which 16 * TT tokens an attention workgroup serves, the members'
// caches and their row ranges.  Passed by value as kernarg; every pointer is device memory.
struct PackedRow { int seq, t; };       // row r: token t (0-based among the call's new tokens) of sequence seq
struct PackedItem { int seq, t0; };     // attention item: tokens [t0, t0 + 16 * TT) of sequence seq (t0 a multiple of 16 * TT)
struct PackedTable {
    const PackedRow *rows = nullptr;    // [T_total]
    const PackedItem *items = nullptr;  // [n_items]
    const SeqRef *seqs = nullptr;       // [n_seq]
    const int *seq_off = nullptr;       // [n_seq] first row of the sequence
    const int *seq_cnt = nullptr;       // [n_seq] its new tokens
    const int *seq_vt = nullptr;        // [n_seq] 1: its value cache is transposed (the MFMA attention layout)
};
// one member's step state at the start of the call (what set_shard_state sets for one cache), and its fused-attention tickets
struct PackedSeqInit { unsigned *heads_done; uint32_t token, pos, len, _pad; SampleState ss; };
// every member's StepState / SampleState / tickets (n_tickets words each) in one launch; init_dev: device array [n_seq]
int launch_packed_set_states(Launcher &L, const PackedTable &tb, const PackedSeqInit *init_dev, int n_seq, int n_tickets);
// out_dev [2 * n_seq]: every member's token (left by token selection) and error word, for one copy to the host
int launch_packed_collect(Launcher &L, const PackedTable &tb, uint32_t *out_dev, int n_seq);
// qkv fp32 [n_slab][T_total][(H+2Hkv)*d] -> slabs summed, bias, RoPE at st->pos + t -> q_out [T_total][H*d], k / v appended at slot
// st->len + t of each row's own cache; dtype: the model's (q_out and the caches)
int launch_rope_kv_packed(Launcher &L, int dtype, const float *qkv, const PackedTable &tb, const float *cos_tab, const float *sin_tab,
                          int64_t max_pos, void *q_out, size_t kv_layer_off, int64_t T_total, int64_t H, int64_t Hkv, int64_t d, int n_slab = 1,
                          const float *bias = nullptr);
// bf16, MFMA layout: causal / sliding-window attention of every item's tokens over their own sequence's cache (mask as
// launch_attn_prefill_mfma, per sequence); q / out [T_total][H*d].  TT, ks: what plan_attn_prefill_packed (attn_prefill_plan.h) chose
// (tb.items were cut for TT); ks 2: the 16-row kernel's wave-pair key split, 1: its plain ring
struct AttnPrefillTune;
AttnPrefillTune attn_prefill_tune();   // the prefill attention plans' switches as tune() has them now (k_attn_mfma.hip)
int launch_attn_prefill_packed_mfma(Launcher &L, const void *q, const PackedTable &tb, int n_items, int TT, int ks, size_t kv_layer_off, void *out,
                                    int64_t H, int64_t Hkv, int64_t d, float scale, int64_t window, double flops = 0, int mask = 0);   // mask 1: full (every token sees all of its sequence's keys, no window)
// The host image of one call's table: the arrays back to back (SeqRef first: it holds pointers), and where each begins.  Items are
// cut, 16 * TT tokens each, for the members with vt[s] != 0 only (the others' attention runs per sequence); TT and ks from
// plan_attn_prefill_packed over those members.
struct PackedHost {
    std::vector<unsigned char> bytes;
    size_t off_seqs = 0, off_rows = 0, off_items = 0, off_off = 0, off_cnt = 0, off_vt = 0;
    int n_seq = 0, n_items = 0, T_total = 0, TT = 1, ks = 1;
    PackedTable at(const void *dev_base) const;           // the table of this image once it lies at dev_base
};
// pad_rows: that many copies of the last row's entry behind the rows (fl_batch_verify's one-row pack); they belong to no member's count
// and to no attention item
void packed_table_build(const SeqRef *refs, const int *counts, const int *vt, int n, int64_t H, int64_t Hkv, int64_t d, PackedHost *out,
                        int pad_rows = 0);
// dst [n_slab][n_seq][h] = the sequences' last rows of src [n_slab][..][h] (slabs src_slab / dst_slab floats apart)
int launch_gather_last_rows(Launcher &L, const float *src, const PackedTable &tb, float *dst, int n_seq, int64_t h, int n_slab, int64_t src_slab,
                            int64_t dst_slab);

// Decoder-model embeddings (k_pool.hip, fl_batch_embed / fl_op_pool_rows): the pooled final hidden states of a pack.
//   hid[t][j] = (x[t][j] * inv_rms[t]) * w[j]      (x, inv_rms: what the final launch_rmsnorm_add leaves; both products rounded)
// pooling FL_POOL_LAST / FIRST: member s's last / first row; MEAN: the sum over its rows in row order from +0, one rounded add per
// row, then one rounded division by (float)count; NONE: every row its own member (seq_off / seq_cnt are not read, n_out = T).
// out [n_out][dims] fp32, dims <= h.  normalize: a second small launch divides every vector by the root of its sum of squares, the
// column chunks' partial sums (part, [n_out][pool_rows_chunks(dims)] floats) added in chunk order; a zero vector stays zero.
int pool_rows_chunks(int64_t dims);
int launch_pool_rows(Launcher &L, const float *x, const float *inv_rms, const float *w, const int *seq_off, const int *seq_cnt, int n_out,
                     int64_t h, int64_t dims, int pooling, bool normalize, float *part, float *out);

// dst row of gate/up pair q in the 16-interleaved fused layout: 16 gate rows then 16 up rows
__host__ __device__ inline int64_t gateup_row(int64_t q, int is_up) { return (q / 16) * 32 + (q % 16) + (is_up ? 16 : 0); }

// ---- projections ---------------------------------------------------------------------------
// y = x[T,K] . W[N,K]^T (+bias).  EPI_F32: y fp32 [T,N].  EPI_GATEUP: W is the 16-interleaved
// gate/up matrix (N = 2*I rows), y is XT [T, I] = silu(gate)*up.
// dtype FL_DTYPE_BF16: W and x (and gate-up y) bf16; FL_DTYPE_F32: all fp32.
// row_scale (optional, fp32 [T]): y[t,:] = row_scale[t] * (x[t,:] . W^T) (+bias) -- the 1/rms factor of
// a preceding RMSNorm, applied after the dot product (see launch_rmsnorm_add).
// max_split > 1 allows split-K: y then holds *n_split_out fp32 slabs of [T,N] that the consumer sums
// (launch_rmsnorm_add does); *n_split_out is always written when the pointer is given.
// captured: the launch may be recorded into a graph (a decode batch's step)
int launch_linear(Launcher &L, int dtype, const void *W, const void *x, const float *bias, void *y,
                  int64_t T, int64_t N, int64_t K, int epi, const float *row_scale = nullptr,
                  int max_split = 1, int *n_split_out = nullptr, bool captured = false);

struct RopeEpi;
// ---- which kernel runs a projection (k_linear.hip): the one place the selection rules are combined.  The per-kernel rules
// (gemm_h4_plan, gemm_skf_plan, gemm_pick_kernel, gemm_peel_plan ...) are its inputs; launch_plan carries a plan out.
enum { LK_NONE, LK_GEMV, LK_H4, LK_W14, LK_SKF, LK_DMA, LK_SKINNY, LK_8P, LK_8P_STREAMK, LK_256, LK_128, LK_4W_ROPE, LK_GENERIC,
       LK_F32_ROWS, LK_F32_MFMA };
struct LinearPlan {
    int kernel = LK_NONE, ks = 1;      // rows [0, rows_main) x columns [0, n_main) in ks K slices (met inside the launch, or slabs)
    int64_t n_main = 0;                // < N: a peeled matrix -- columns [n_main, N) on `tail`, the same rows
    int tail = LK_NONE, tail_ks = 1;
    int64_t rows_main = 0;             // < T: a gate/up row split -- rows [rows_main, T) on `rest`, all columns
    int rest = LK_NONE, rest_ks = 1;
    int n_split = 1;                   // fp32 slabs the output is left in (the consumer sums them)
    bool rope = false;                 // plan_qkv_rope: RoPE / bias / KV append in the epilogue; false: fp32 output for launch_rope_kv
    bool reads_rs_parts = false;       // every launch takes its row scales from Launcher::rsp (the caller may leave them as partial sums)
};
// takes_slabs: the caller sums up to max_split fp32 slabs; tp: the model's tensor-parallel degree (> 1: a rank's shard shapes)
LinearPlan plan_linear(int dtype, int64_t T, int64_t N, int64_t K, int epi, int tp, int max_split, bool bias, bool takes_slabs, bool captured);
// o_proj / down_proj with the residual epilogue (EPI_RESID); kernel LK_NONE: keep the rmsnorm_add launches
LinearPlan plan_resid(int dtype, int64_t T, int64_t N, int64_t K, int max_split, bool captured);
// the QKV projection of a prompt; kv_width: the k (= v) columns of this shard
LinearPlan plan_qkv_rope(int dtype, int64_t T, int64_t N, int64_t K, int64_t d, int64_t kv_width, int tp, int max_split);
int launch_plan(Launcher &L, const LinearPlan &p, int dtype, const void *W, const void *x, const float *bias, void *y, int64_t T, int64_t N,
                int64_t K, int epi, const float *row_scale, const ResidEpi *re = nullptr, const RopeEpi *ro = nullptr);
// planner inputs of the tiled kernels (k_gemm_mfma.hip): the cost model's pick (LK_8P / LK_256 / LK_128), the same under FL_GEMM_8P
int gemm_pick_kernel(int64_t T, int64_t N, int64_t K, int ks, double *cost_out = nullptr);
int gemm_tile_kernel(int64_t T, int64_t N, int64_t K, int epi, bool bias, int ksplit, bool allow8p);
int gemm_mfma_ksplit(int64_t T, int64_t N, int64_t K, int epi, int max_split);
bool gemm_streamk_whole(int64_t T, int64_t N, int64_t K);
bool gemm_peel_plan(int64_t T, int64_t N, int64_t K, int64_t *n_main_out);
bool gemm_resid_8p_wins(int64_t T, int64_t N, int64_t K, int max_split);
int gemm_resid_partials(int64_t N);                                                       // partial sums per row (np)
// ldc: row stride of y in elements of the FULL output width (0 = N): a launch may cover a column range of a wider matrix
int launch_gemm_mfma(Launcher &L, bool wide, const void *W, const void *x, const float *bias, void *y,
                     int64_t T, int64_t N, int64_t K, int epi, const float *row_scale, int ksplit, int64_t ldc);
int launch_rms_finalize(Launcher &L, const float *part, int np, float eps, float *inv_rms, int64_t T, int64_t h);
// Every launch of a kernel that reads its row scales as a VECTOR first finishes Launcher::rsp's partial sums into row_scale: the safety
// net under a caller that sets rsp where the plan did not say reads_rs_parts (FL_DEBUG_RS_PARTS: on purpose).
int rs_parts_to_vector(Launcher &L, const float *row_scale, int64_t T);
int64_t gemm_8p_workspace_bytes(hipStream_t stream);   // stream-K workspace held for a stream on the current device
void gemm_8p_release_stream(hipStream_t stream);   // frees the stream-K workspace of a stream that is about to be destroyed
int launch_gemm_8p(Launcher &L, const void *W, const void *x, const float *bias, void *y, int64_t T, int64_t N, int64_t K,
                   int epi, const float *row_scale, int ksplit, int64_t ldc = 0, bool streamk = false, const ResidEpi *resid = nullptr);
// EPI_QKV_ROPE (k_gemm_h4.hip): the QKV projection's epilogue applies the row scale and bias, rotates q / k and appends k / v to the
// cache -- what launch_rope_kv does behind a plain fp32 output
struct RopeEpi {
    int on = 0;
    const StepState *st = nullptr;
    const float *cos_tab = nullptr, *sin_tab = nullptr;
    int max_pos = 0;
    void *q_out = nullptr, *k_cache = nullptr, *v_cache = nullptr;     // bf16: q [T][H*d]; K [Hkv][max_seq][d]; V [Hkv][d][max_seq] (transposed) or as K
    int H = 0, Hkv = 0, d = 0, max_seq = 0, v_transposed = 0;
    int col_base = 0;                  // first column of this launch in the whole QKV matrix (a column-peeled projection's tail launch)
    // decode batch (k_gemm_skf.hip only): row t is sequence t's single new token -- its RoPE position, KV slot and caches come from
    // seqs[t] (st->pos, st->len, k / v + kv_layer_off * seq_alloc; V transposed), not from st / k_cache / v_cache
    const struct SeqRef *seqs = nullptr;
    size_t kv_layer_off = 0;
};
// 128 x 256 tile, K slices summed inside the launch (k_gemm_h4.hip): mid-size prompts
constexpr int H4_MAXS = 4;             // K slices at most
struct H4Space {
    float *part;                       // [tile][slice][128 x 256] fp32 partial accumulators, lane-major
    unsigned *ctr;                     // [2 sets][tile]{slices published, flag word: abandoned blocks' bits | CLOSED}: alternate launches use alternate sets and zero the other
};
bool gemm_h4_supported(int64_t T, int64_t N, int64_t K, int ksplit);
int gemm_h4_plan(int64_t T, int64_t N, int64_t K, int epi);
int gemm_h4_plan_whole(int64_t T, int64_t N, int64_t K, int epi);   // ... for a caller that needs one complete output (no slabs): a tensor-parallel rank's projections
// 256 x 224 four-wave tile (k_gemm_w14.hip): fp32 / gate-up epilogues, N whole 224-column tiles
// fp32 operands on the matrix cores (k_gemm_f32.hip): the fp32 mode's prompt GEMM, bit-identical to gemm_generic_kernel's fmaf chains
bool gemm_f32_mfma_supported(int64_t T, int64_t N, int64_t K);
// fp32, 2-64 token rows: a weight stream with the x rows in LDS (k_gemm_f32.hip)
bool gemv_f32_rows_supported(int64_t T, int64_t N, int64_t K, int epi);
int launch_gemv_f32_rows(Launcher &L, const void *W, const void *x, const float *bias, void *y, int64_t T, int64_t N, int64_t K, int epi,
                         const float *row_scale);
int launch_gemm_f32_mfma(Launcher &L, const void *W, const void *x, const float *bias, void *y, int64_t T, int64_t N, int64_t K,
                         int epi, const float *row_scale);
bool gemm_w14_plan(int64_t T, int64_t N, int64_t K, int epi);
// the four-wave 256 x 256 kernel with the RoPE / bias / KV-append epilogue (k_gemm_8p.hip): a long prompt's QKV projection, whole K
bool gemm_4w_rule(int64_t T, int64_t N, int64_t K, int64_t ksteps, bool streamk);
bool gemm_4w_rope_supported(int64_t T, int64_t N, int64_t K);
int launch_gemm_4w_rope(Launcher &L, const void *W, const void *x, const float *bias, int64_t T, int64_t N, int64_t K, const float *row_scale,
                        const RopeEpi &rope);
int launch_gemm_w14(Launcher &L, const void *W, const void *x, const float *bias, void *y, int64_t T, int64_t N, int64_t K,
                    int epi, const float *row_scale, int64_t ldc = 0);
int gemm_h4_tail_slices(int64_t T, int64_t N, int64_t K);     // a peeled GEMM's tail columns on this kernel: K slices, or 0 = the stream-K launch + fix-up
int launch_gemm_h4(Launcher &L, const void *W, const void *x, const float *bias, void *y, int64_t T, int64_t N, int64_t K,
                   int epi, const float *row_scale, int ksplit, int64_t ldc = 0, const ResidEpi *resid = nullptr, const RopeEpi *rope = nullptr);
int64_t gemm_h4_workspace_bytes(hipStream_t stream);
// short prompts and decode batches (2-128 rows, k_gemm_skf.hip): the weight-streaming GEMM with its K slices met inside the launch and the
// fp32 / gate-up / residual + norm / RoPE + KV-append epilogues; d: head_dim of the RoPE epilogue (0 otherwise)
int gemm_skf_plan(int64_t T, int64_t N, int64_t K, int epi, int d = 0);
int launch_gemm_skf(Launcher &L, const void *W, const void *x, const float *bias, void *y, int64_t T, int64_t N, int64_t K, int epi,
                    const float *row_scale, int ksplit, const ResidEpi *resid = nullptr, const RopeEpi *rope = nullptr);
void gemm_skf_release_stream(hipStream_t stream);
void gemm_h4_release_stream(hipStream_t stream);   // before the owner destroys the stream
bool gemm_skinny_supported(int64_t T, int64_t N, int64_t K);
int gemm_skinny_ksplit(int64_t T, int64_t N, int64_t K, int epi, int max_split);
int launch_gemm_skinny(Launcher &L, const void *W, const void *x, const float *bias, void *y, int64_t T, int64_t N, int64_t K,
                       int epi, const float *row_scale, int ksplit);
// cheap capability probes used by tests / DESIGN numbers
bool gemv_supported(int dtype, int64_t N, int64_t K);
bool gemm_mfma_supported(int dtype, int64_t T, int64_t N, int64_t K);

// ---- small ops -----------------------------------------------------------------------------
// x_res[t,:] = E[ids[t],:]; ids == nullptr: single token read from st->token
int launch_embed(Launcher &L, int dtype, const void *E, const uint32_t *ids, const StepState *st,
                 float *x_res, int64_t T, int64_t h);
// x_res += delta (if delta); xs = x_res * w (compute dtype); inv_rms[t] = 1/sqrt(mean(x_res^2)+eps).
// RMSNorm(x) * w == inv_rms * xs: the scalar is applied by the consuming projection's epilogue, so
// the bf16 rounding point (xs) is the same in the prefill and the fused decode path.
// delta may be n_slab split-K slabs, slab s at delta + s * slab_stride floats.
int launch_rmsnorm_add(Launcher &L, int dtype, float *x_res, const float *delta, const float *w,
                       float eps, void *xs, float *inv_rms, int64_t T, int64_t h, int n_slab = 1,
                       int64_t slab_stride = 0);
// RoPE(q,k) + KV append.  qkv fp32 [T, (H+2Hkv)*d]; q_out XT [T,H*d]; caches XT [Hkv][max_seq][d]
// v_transposed: value cache laid out [Hkv][d][max_seq] instead of [Hkv][max_seq][d]
int launch_rope_kv(Launcher &L, int dtype, const float *qkv, const StepState *st, const float *cos_tab,
                   const float *sin_tab, int64_t max_pos, void *q_out, void *k_cache, void *v_cache,
                   int64_t T, int64_t H, int64_t Hkv, int64_t d, int64_t max_seq, bool v_transposed, int nslab = 1,
                   const float *bias = nullptr);   // bias: the QKV projection's, when it ran in K slices (added after the slabs are summed)
// (nslab > 1: qkv is nslab split-K slabs of [T][(H+2Hkv)*d], summed here in slab order)
bool rope_kv_takes_vec(int dtype, bool v_transposed, int64_t T, int64_t d, int64_t max_seq);   // launch_rope_kv's rule for rope_kv_vec_kernel
// logits[V] -> st->token by ArgMax (ties: last max index) or, when ss->on, by temperature sampling with
// the seeded ChaCha12 stream; out_tokens[st->step] = token; advances pos/len/step
int launch_select_advance(Launcher &L, const float *logits, int64_t V, StepState *st, SampleState *ss, float *scratch /* [V] */,
                          uint32_t *out_tokens, int advance,
                          const ArgmaxCand *cand = nullptr /* the lm_head launch's candidates: ArgMax without reading the vocabulary again */,
                          uint32_t *epoch_bump = nullptr /* the decode engine's tag epoch: += 1 per forward */);
// fl_forward_verify's selection: logits [T][V] -> out[t] = ArgMax of row t (ties: last max index), out[kVerifyNacc] = how many of
// draft[0 .. T-1) the rows confirm (draft[i] == out[i] for all i below it).  out: kVerifyWords words, zero before the FIRST launch
// (the ticket word is put back by the kernel itself)
constexpr int kVerifyMaxRows = 16, kVerifyNacc = 16, kVerifyTicket = 17, kVerifyWords = 18;
int launch_verify_select(Launcher &L, const float *logits, int64_t V, int T, const uint32_t *draft /* [T-1] device */, uint32_t *out);
// fl_forward_verify_ex's selection: out[t] = the draw of row t -- select_advance's sampler with word (ss.draw_hi:draw_lo) + t of the
// seeded stream -- and the same acceptance scan, ticket and out block.  ss.on != 0 (ArgMax is launch_verify_select's); scratch:
// [T][V] floats; kept (device, or null): [T] what the top-p / top-k filter kept per row (V without one).
int launch_verify_sample(Launcher &L, const float *logits, int64_t V, int T, const uint32_t *draft /* [T-1] device */, const SampleState &ss,
                         float *scratch, uint32_t *out, uint32_t *kept);
// fl_batch_verify's selection (k_verify_packed.hip): the verify steps of up to 64 members, 1..16 rows each, as the rows of ONE pack of
// T_total <= 1024 rows.  logits [R][V] holds rows r0 .. r0 + R of the pack (one lm_head block); row r is token rows[r].t of member
// rows[r].seq and is selected as that member's SampleState says -- on == 0: ArgMax as launch_verify_select; else the draw of
// launch_verify_sample with word (draw_hi:draw_lo) + t -- so one launch may mix the two.  Each member has its own acceptance scan and
// ticket word in out, and a member whose rows straddle two launches is completed by the later one (same stream).
// out: [0, T_total) the ids | [kVerifyPackedNacc + s] member s's accepted count | [kVerifyPackedAux ..) free for the caller (the
// members' error words, fl_batch_verify) | [kVerifyPackedTicket + s] its ticket; kVerifyPackedWords words, zero before the FIRST launch.
constexpr int kVerifyPackedMaxRows = 1024, kVerifyPackedNacc = 1024, kVerifyPackedAux = 1088, kVerifyPackedTicket = 1216, kVerifyPackedWords = 1280;
struct VerifyPackedArgs {                // every pointer is device memory
    const PackedRow *rows = nullptr;     // [T_total]
    const int *seq_off = nullptr;        // [n_seq] a member's first row
    const int *seq_cnt = nullptr;        // [n_seq] its rows, 1..16
    const SampleState *ss = nullptr;     // member s's state lies s * ss_stride BYTES behind this one (an array of SampleState or of PackedSeqInit)
    size_t ss_stride = sizeof(SampleState);
    const uint32_t *ids = nullptr;       // [T_total] the pack's ids: a member's token, then its draft
    uint32_t *out = nullptr;
    uint32_t *kept = nullptr;            // [T_total] or null: what the top-p / top-k filter kept per row (V without one, and for ArgMax rows)
};
// scratch: [R][V] floats, needed (any_sampled) when a member of the pack samples
int launch_verify_packed(Launcher &L, const float *logits, int64_t V, int r0, int R, int T_total, const VerifyPackedArgs &a, float *scratch,
                         bool any_sampled);
// fl_*_lp: log-softmax (temperature 1, no mask) of `rows` logits rows [rows][V], one workgroup per row -- the chosen token's and the
// first top_n of "logit descending, lower index first" -- into record `step - advance` of the row's LogprobCtl.  Who a row belongs to:
//   st + ctl      one sequence (rows == 1): the token select_advance just left in st
//   seqs + ctls   a batch: row b is sequence b (its SeqRef's StepState, ctls[b])
//   chosen + ctl  fl_op_logprobs: row t's token is chosen[t], its record ctl->recs[t]
struct LogprobSrc {
    const StepState *st = nullptr;
    const SeqRef *seqs = nullptr;
    const LogprobCtl *ctl = nullptr;
    const LogprobCtl *const *ctls = nullptr;
    const uint32_t *chosen = nullptr;
};
int launch_token_logprobs(Launcher &L, const float *logits, int64_t V, int rows, const LogprobSrc &src, int advance);
int launch_set_logprob_ctl(Launcher &L, LogprobCtl *ctl, LogprobRec *recs, uint32_t cap, int top_n);
// fl_forward_score / fl_batch_score / fl_op_score (k_score.hip): the same log-softmax of `rows` logits rows [rows][V], one workgroup per
// row, against targets[row] (device; >= V: no target) -- its log-prob, its rank in the order, and the first top_n -- into recs[row]
int launch_score_rows(Launcher &L, const float *logits, int64_t V, int rows, const uint32_t *targets, int top_n, ScoreRec *recs);
// Logit rules (k_logit_rules.hip): out row b = the rules of row b's control block applied to logits row b ([rows][V], fp32), one
// launch between lm_head and token selection.  The thread that owns element `token` of a row first counts it (count_input).  Who a
// row belongs to:
//   st + ctl          one sequence (rows == 1): token st->token, output ctl->out
//   seqs + ctls + out a batch: row b is sequence b (its SeqRef's StepState, ctls[b]; a null entry copies the row through), out [B][V]
//   tokens + ctls + out   fl_op_logit_rules: row b's token is tokens[b] (>= V: none)
struct LogitRulesSrc {
    const StepState *st = nullptr;
    const SeqRef *seqs = nullptr;
    const LogitRulesCtl *ctl = nullptr;
    const LogitRulesCtl *const *ctls = nullptr;
    const uint32_t *tokens = nullptr;
    float *out = nullptr;
};
int launch_logit_rules(Launcher &L, const float *logits, int64_t V, int rows, const LogitRulesSrc &src);
int launch_set_logit_rules_ctl(Launcher &L, LogitRulesCtl *ctl, const LogitRulesCtl &value);
// Guided decoding (k_guide.hip): out row b = logits row b with -inf outside the token list of row b's automaton state, one launch
// between lm_head (or the rules launch) and token selection; logits and out must be different buffers.  At a step > 0 the state first
// moves along the edge of the row's input token.  Who a row belongs to:
//   st + ctl          one sequence (rows == 1): step and token of st, output ctl->out
//   seqs + ctls + out a batch: row b is sequence b (its SeqRef's StepState, ctls[b]; a null entry copies the row through), out [B][V]
//   tokens + ctls + out   fl_op_guide_mask: row b moves from ctls[b]->state[1] along tokens[b] (no edge, or >= V: it stays); the state
//                     the row was masked in comes back in ctls[b]->state[0]
struct GuideSrc {
    const StepState *st = nullptr;
    const SeqRef *seqs = nullptr;
    GuideCtl *ctl = nullptr;
    GuideCtl *const *ctls = nullptr;
    const uint32_t *tokens = nullptr;
    float *out = nullptr;
};
int launch_guide_mask(Launcher &L, const float *logits, int64_t V, int rows, const GuideSrc &src);
int launch_set_guide_ctl(Launcher &L, GuideCtl *ctl, const GuideCtl &value);
// Rules and guide inside a verify step (k_verify_adjust.hip): out row i = logits row i ([T][V] fp32, T <= kVerifyMaxRows) adjusted with
// the table AS IT STANDS AFTER THE INPUTS OF ROWS 0..i -- the table itself is only read: each table word is counted once per r <= i
// with ids[r] == its id -- and masked in states[i].  Everything a row needs travels by value, so a packed form can pass other rows'.
// table null: no rules (allowed ids keep their bits); row_ptr null: no guide; one of the two must be there.  out != logits.
struct VerifyAdjustArgs {
    uint32_t ids[kVerifyMaxRows] = {};       // row i's input id: the step's token, then its drafts (>= V: counts nothing)
    uint32_t states[kVerifyMaxRows] = {};    // the guide state row i is masked in (< n_states: the caller's duty)
    const LogitRuleEntry *table = nullptr;   // [V]
    float rp = 1.f, fp = 0.f, pp = 0.f;
    const uint64_t *row_ptr = nullptr;       // the guide's CSR arrays (GuideCtl's)
    const uint32_t *tokens = nullptr;
    float *out = nullptr;                    // [T][V]
};
int launch_verify_adjust(Launcher &L, const float *logits, int64_t V, int T, const VerifyAdjustArgs &a);
// ... and behind the step's selection: ids[0 .. n) counted into the table, in order (an id twice: counted twice; >= V: nothing)
struct RulesCountArgs { uint32_t ids[kVerifyMaxRows] = {}; int n = 0; };
int launch_rules_count(Launcher &L, LogitRuleEntry *table, int64_t V, const RulesCountArgs &a);
// dst[i] = sum_s src[s][i] for n floats, written to every src (emulated all-reduce)
int launch_reduce_shards(Launcher &L, float *const *bufs_dev, int nshards, int64_t n);

// ---- one-shot collectives over peer-mapped HBM (k_comm.hip) -----------------------------------
constexpr int FL_MAX_TP = 8;
// Per-rank view of the tp inboxes: entry r is rank r's inbox / flag array as mapped in THIS process
// (own allocation for r == rank, hipIpcOpenMemHandle / peer pointer otherwise).
struct CommTable {
    float *inbox[FL_MAX_TP]; uint32_t *flags[FL_MAX_TP];
    int loop = 0;        // 1: LOOPBACK (tools/tp_rank_loopback.py, TK_DEBUG_TP_LOOPBACK): every entry is this rank's own inbox and the kernel plays all
                         // tp ranks' pushes itself -- one rank's step timed with its exchange in place, results meaningless
};
int launch_oneshot(Launcher &L, bool gather, const float *in, float *out, const CommTable &tab, int rank, int tp,
                   int64_t n, int64_t nmax, int64_t out_stride, uint32_t *epoch_ctr, uint32_t *err, long long timeout_ticks,
                   uint32_t *abort_flag = nullptr, uint32_t *done_ctr = nullptr, int max_wgs = 0);     // done_ctr: a zeroed device word, max_wgs > 1 -> large messages go over up to max_wgs workgroups

// All-reduce fused into the epilogue of a row-parallel decode GEMV ("LL" protocol: a value and the epoch that
// validates it travel in ONE 8-byte store, so there is no fence, no flag round and no separate kernel).  Every
// wave pushes its rows' partial sums into slot [rank] of every peer's LL region, polls the tp slots of its own
// region for the same rows and adds them in rank order -- bit-identical to oneshot_kernel's sum.
// Region layout (uint64 {lo: fp32 bits, hi: epoch}): [2 halves by epoch parity][tp source ranks][n rows].
// epoch = *epoch_ctr * slots + slot: the one-shot counter moves at least once per decode step (logits gather).
struct LLTable {
    uint64_t *peer[FL_MAX_TP];      // rank r's LL region as mapped here
    const uint32_t *epoch_ctr;      // the one-shot collectives' device counter
    uint32_t *err;                  // pinned host word
    uint32_t *abort_flag;           // device word, set with err: later waits of a broken step give up after ~1 ms
    long long timeout_ticks;
    int rank, tp, n, slots;
    int loop;                       // 1: loopback (see CommTable::loop): lane p pushes into slot [p] of its own region
};
// stand-alone exerciser of ll_allreduce_rows (bootstrap self-test, tests): out[i] = sum_r in_r[i], i < n
int launch_ll_allreduce(Launcher &L, const LLTable *ll_dev, int slot, const float *in, float *out, int64_t n);

// ---- attention -----------------------------------------------------------------------------
struct AttnScratch {
    float *part_m, *part_l, *part_o; unsigned *counters; int nsplit; int64_t kv_len_hint;
    // decode (k_attn_mfma.hip): bytes the NEXT launch will stream (the layer's o_proj weights), touched by extra workgroups of
    // this launch while its own few MB leave HBM idle -- they are then served from the Infinity Cache
    // (prefetch_chunk: the bytes one workgroup of that launch reads contiguously, gemv_owner_chunk)
    const void *prefetch = nullptr; int64_t prefetch_bytes = 0, prefetch_chunk = 0, prefetch_row = 0;   // (row: bytes of one matrix row)
};
// decode: one query token over len+1 cached keys, no mask (App. A.5)
int launch_attn_decode(Launcher &L, int dtype, const void *q, const void *k_cache, const void *v_cache,
                       const StepState *st, void *out, const AttnScratch &sc, int64_t H, int64_t Hkv,
                       int64_t d, int64_t max_seq, float scale);
// prefill: T queries; key kj visible to query t iff kj < len, or (j=kj-len) j<=t and j+window>=t
int launch_attn_prefill(Launcher &L, int dtype, const void *q, const void *k_cache, const void *v_cache,
                        const StepState *st, void *out, int64_t T, int64_t H, int64_t Hkv, int64_t d,
                        int64_t max_seq, float scale, int64_t window, int mask = 0);   // mask 1: full -- every query sees all len + T keys, no window

// bf16 MFMA attention (k_attn_mfma.hip): needs the transposed value cache [Hkv][d][seq_alloc], seq_alloc % 32 == 0
bool attn_mfma_supported(int dtype, int64_t H, int64_t Hkv, int64_t d);
int launch_attn_decode_mfma(Launcher &L, const void *q, const void *k_cache, const void *v_cache_T, const StepState *st,
                            void *out, const AttnScratch &sc, int64_t H, int64_t Hkv, int64_t d, int64_t seq_alloc,
                            float scale);
int launch_attn_prefill_mfma(Launcher &L, const void *q, const void *k_cache, const void *v_cache_T, const StepState *st,
                             void *out, int64_t T, int64_t H, int64_t Hkv, int64_t d, int64_t seq_alloc, float scale,
                             int64_t window);
// test hook (fl_op_attention): 0 = pick by prompt length, 2 = the 16-row kernel, 3 = the 32-row kernel
void attn_prefill_force(int which);

// decode attention + o_proj in one launch (k_attn_oproj.hip): W_o is pulled into LDS while attention runs; the output is one
// partial vector per kv head
bool attn_oproj_plan(int64_t H, int64_t Hkv, int64_t d, int64_t h, int nsplit, int cus, int *n_blocks, int *rows_attn,
                     int *rows_other, size_t *lds_bytes);
int launch_attn_oproj(Launcher &L, const void *q, const void *k_cache, const void *v_cache_T, const StepState *st,
                      StepState *st_rw, float *partials /* [H][nsplit][d + 4] */, unsigned *done /* [Hkv] words of this layer */,
                      int nsplit, int attn_waves /* 1..8: 32 keys each per split and step */, int64_t kv_len_hint, const void *Wo, float *slabs /* [Hkv][h] */, int64_t H, int64_t Hkv, int64_t d,
                      int64_t h, int64_t seq_alloc, float scale);

// decode attention + o_proj in one launch for SHORT caches (k_attn_rep.hip): every workgroup computes the attention of all heads
// itself (K / V from L2) while its rows of W_o stream in; out = W_o . attention (fp32 [N]), or summed over the ranks (ll)
struct AttnRepArgs {
    const void *q = nullptr, *kc = nullptr, *vT = nullptr;     // q [H*d] bf16; K cache [Hkv][seq_alloc][d]; V^T cache [Hkv][d][seq_alloc]
    const StepState *st = nullptr;
    const void *Wo = nullptr;                                  // [N, K = H*d] bf16
    float *out = nullptr;
    int H = 0, Hkv = 0, seq_alloc = 0, N = 0, K = 0;
    float scale = 0.f;
    const LLTable *ll = nullptr; int ll_slot = 0;
};
bool attn_oproj_rep_supported(int64_t H, int64_t Hkv, int64_t d, int64_t h, int64_t max_seq, bool any_size = false);
// rows per wave, head slots per slab (GMAX), workgroups, slices per kv head and dynamic LDS of a launch with N rows; and whether a cache
// of seq_alloc rows passes the model's rule / the any-size rule
struct AttnRepGeometry { int rpw = 0, gmax = 0, blocks = 0, nslice = 0; size_t lds = 0; bool model_rule = false, any_size = false; };
bool attn_oproj_rep_geometry(int64_t H, int64_t Hkv, int64_t d, int64_t N, int64_t seq_alloc, AttnRepGeometry *g);
int launch_attn_oproj_rep(Launcher &L, const AttnRepArgs &a);

// ---- the BERT / MiniLM encoder (k_encoder.hip): a packed, ragged batch of sequences -- row r of every [T_total][..] buffer belongs to
// sequence row_seq[r], which owns rows [offsets[s], offsets[s + 1]) ------------------------------------------------------------------
enum { ENC_ACT_NONE = -1, ENC_ACT_GELU_TANH = 0, ENC_ACT_GELU_ERF = 1 };
// LayerNorm with bias, candle_nn::LayerNorm: (x - mean) / sqrt(biased var + eps) * w + b, statistics in fp32
// x = LN(word[ids[r]] + pos[r - offsets[row_seq[r]]] (+ tt0)) -> x_res fp32 [T][h] and xn (compute dtype) [T][h]; tables in `dtype`
int launch_encoder_embed_ln(Launcher &L, int dtype, const void *word, const void *pos, const void *tt0 /* [h] or null */, const uint32_t *ids,
                            const int32_t *row_seq, const int32_t *offsets, const float *w, const float *b, float eps, float *x_res, void *xn,
                            int64_t T, int64_t h);
// x_res = LN(x_res + sum of the n_slab split-K slabs of delta (+ bias, when the projection did not add it)) -> x_res and xn
int launch_encoder_add_ln(Launcher &L, int dtype, float *x_res, const float *delta, int n_slab, int64_t slab_stride, const float *bias,
                          const float *w, const float *b, float eps, void *xn, int64_t T, int64_t h);
// out (compute dtype) [T][N] = act(sum of slabs of y fp32 [T][N] (+ bias)); act ENC_ACT_NONE: the conversion alone (Q | K | V)
int launch_encoder_bias_act(Launcher &L, int dtype, const float *y, int n_slab, int64_t slab_stride, const float *bias, int act, void *out,
                            int64_t T, int64_t N);
// unmasked softmax attention of every (sequence, head): q / k / v rows are ld elements apart (a [T][3h] buffer: ld = 3h), out [T][H*d]
// in the compute dtype.  bf16: MFMA kernel, 64 query rows per workgroup, keys streamed through LDS in tiles of 32; fp32: one wave per
// query row.  d 32 or 64; ld a multiple of 8.  max_len: the longest sequence (sizes the grid)
bool encoder_attention_supported(int64_t d);
int launch_encoder_attention(Launcher &L, int dtype, const void *q, const void *k, const void *v, int64_t ld, const int32_t *offsets, int64_t n_seq,
                             int64_t max_len, int64_t T_total, int64_t H, int64_t d, float scale, void *out);
// out[s][:] = mean over the sequence's rows of x (fp32, row order), divided by its L2 norm
int launch_encoder_pool_l2(Launcher &L, const float *x, const int32_t *offsets, int64_t n_seq, int64_t h, float *out);

// ---- weight conversion at model build ---------------------------------------------------------
// dst[row_map(r)][c] = cvt(src[r0+r][c0+c]); row_mode 0: dst_row0+r, 1: gate rows, 2: up rows
// via_bf16 (fp32 destinations): the value is rounded to bf16 first -- the fp32 copy of a tensor that the model holds in bf16
int launch_convert_slice(Launcher &L, int src_dtype, const void *src, int64_t src_ld, int64_t r0, int64_t c0,
                         int64_t rows, int64_t cols, int dst_dtype, void *dst, int64_t dst_ld,
                         int64_t dst_row0, int row_mode, int head_pad = 0, int64_t dm = 1, int64_t d = 1, int via_bf16 = 0);   // head_pad: padded head_dim (weights.hip)
int launch_convert_vec_f32(Launcher &L, int src_dtype, const void *src, int64_t off, int64_t n, float *dst);

}  // namespace fl
