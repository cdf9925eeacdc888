// model.h -- model / cache objects behind the C ABI and the forward-pass orchestration.
#pragma once
#include <atomic>
#include <functional>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include <rccl/rccl.h>

#include "kernels.h"

namespace fl {

struct Dims {                    // resolved config (defaults applied)
    int family = 0, qkv_bias = 0;
    int64_t h = 0, inter = 0, V = 0, L = 0, H = 0, Hkv = 0, max_pos = 0, window = -1;
    int64_t dm = 0;              // the MODEL's head_dim = hidden_size / num_attention_heads (any even value, config.rs:31-43)
    int64_t d = 0;               // the head_dim the kernels run: dm padded to 64 or 128 with zero weight rows (weights.hip, build_weights)
    float eps = 0.f, scale = 0.f;
    double theta = 10000.0;
};

int resolve_config(const fl_config *cfg, Dims *out);
int tp_slice(const Dims &D, const char *name, int rank, int tp, int64_t out[4]);

struct LayerW {
    void *wqkv = nullptr;        // [(Hs+2Hkvs)*d, h]  q | k | v rows of this shard
    float *bqkv = nullptr;       // [(Hs+2Hkvs)*d] or null
    void *wo = nullptr;          // [h, Hs*d]
    void *wgu = nullptr;         // [2*Ip, h] 16-interleaved gate/up rows
    void *wd = nullptr;          // [h, Ip]
    float *ln1 = nullptr, *ln2 = nullptr;
    // FL_WEIGHTS_E4M3_ROW: the e4m3 bytes (same shape and row layout) and the per-row scales of the four matrices; the pointers
    // above then hold the bf16 image s * q
    uint8_t *wqkv8 = nullptr, *wo8 = nullptr, *wgu8 = nullptr, *wd8 = nullptr;
    float *sqkv = nullptr, *so = nullptr, *sgu = nullptr, *sd = nullptr;
};

struct Scratch {                 // activations of one forward chunk on one shard
    int64_t cap_T = 0;
    float *x_res = nullptr;      // [T,h] fp32 residual stream
    float *x_res2 = nullptr;     // decode only: ping-pong partner of x_res for the fused norm prologue
    float *delta = nullptr;      // [T,h] fp32 output of o_proj / down_proj (all-reduced under TP)
    void *xn = nullptr;          // [T,h] x * norm_weight (compute dtype); RMSNorm = inv_rms * xn
    float *inv_rms = nullptr;    // [T]
    float *rs_part = nullptr;    // [T, np] partial sums of squares left by the residual epilogue of a long prompt's o_proj / down_proj
    float *qkv = nullptr;        // [T,(Hs+2Hkvs)*d] fp32
    void *q = nullptr;           // [T,Hs*d]
    void *ao = nullptr;          // [T,Hs*d] attention output
    void *act = nullptr;         // [T,Ip] silu(gate)*up
    uint32_t *ids = nullptr;     // [T]
    // decode only: what an o_proj / down_proj with the residual epilogue leaves for the projection behind the next norm
    void *xs_res = nullptr;      // [h] bf16: (x_res + delta) * norm_weight
    float *cs_res = nullptr;     // [h/8] sums of squares of x_res + delta per 8 elements
};

// One-shot collectives over peer-mapped HBM (k_comm.hip): this rank's inbox and its view of the peers'.
struct PeerComm {
    void *local = nullptr;       // hipDeviceMallocUncached: [flags, 4 KB | inbox: 2 halves x tp slots x nmax floats | LL: 2 x tp x h x 8 B]
    size_t bytes = 0;
    int64_t nmax = 0;            // floats per slot
    CommTable tab{};
    void *mapped[FL_MAX_TP] = {};     // hipIpcOpenMemHandle mappings of the peers (closed on destroy)
    uint32_t *epoch = nullptr;   // device: collectives done so far (same on every rank)
    uint32_t *err = nullptr;     // pinned host word a kernel writes when a peer never showed up
    long long timeout_ticks = 0; // wall_clock64 ticks (100 MHz)
    bool connected = false;
    // all-reduce fused into the row-parallel decode GEMVs (comm_ll.h): a region behind the inbox halves
    size_t ll_off = 0;           // byte offset of the LL region in `local` (same on every rank)
    LLTable ll{};                // host copy; `ll_dev` is what the kernels read
    LLTable *ll_dev = nullptr;
    bool ll_ok = false;          // region connected (and, with RCCL, proven against ncclAllReduce by all ranks)
    bool loopback = false;       // TK_DEBUG_TP_LOOPBACK: all entries are this rank's own inbox, the kernels play every rank's push
    bool wide_ok = true;         // messages of 16 384 floats and more over many workgroups (oneshot_wide_kernel): proved at bootstrap, like the rest
    bool shares_device = false;  // a peer lives on this same GPU (rehearsals): full-chip grids that wait for each other cannot co-reside
};

// fl_batch_prefill (prefill_packed.hip): the per-call device table and the last rows' buffers of a packed prefill.  They belong
// to the model, grow with the largest call seen and are freed with it.
struct PackedScratch {
    void *tab = nullptr; size_t tab_bytes = 0;     // device image of the call's PackedHost, the members' PackedSeqInit behind it
    unsigned char *host_tab = nullptr; size_t host_tab_bytes = 0;   // ... and its pinned source
    int cap_n = 0;                                 // sequences the buffers below hold
    float *xl = nullptr;                           // [n][h] the members' last residual rows
    float *dl = nullptr;                           // [kMaxKSplitMid][n][h] ... and their delta slabs
    void *xnl = nullptr; float *inv_rms = nullptr; // [n][h] / [n] the final norm over them
    float *logits = nullptr;                       // [n][V]
    uint32_t *result = nullptr;                    // [64][2] the members' tokens and error words, gathered for one copy
    uint32_t *host_result = nullptr;               // ... pinned
    // fl_batch_verify: the selection launches' block (launch_verify_packed: ids, accepted counts, the members' error words, tickets;
    // zeroed once at allocation; memset again only on a failed call's way out), its pinned image, and -- allocated at a model's first SAMPLED
    // packed verify, regrown with the score_rows switch, counted in hbm_bytes -- the rows' probabilities [verify_prob_R][V]
    uint32_t *verify_out = nullptr;
    uint32_t *host_verify = nullptr;
    float *verify_prob = nullptr; int64_t verify_prob_R = 0;
    // fl_batch_embed: the pooled vectors [embed_rows][h] fp32 and the column chunks' partial sums of squares [embed_rows][chunks];
    // allocated at a model's first embed call, regrown with the largest call, counted in hbm_bytes
    float *embed_out = nullptr, *embed_part = nullptr; size_t embed_rows = 0;
    std::vector<void *> allocs;
};

// fl_forward_score / fl_batch_score: the [R][V] block the rows' logits land in, and a call's targets and records.  They belong to
// the model, are allocated at its first scoring call (and grow with the largest switch value / call seen), are counted in hbm_bytes
// and freed with it.
struct ScoreScratch {
    int64_t cap_R = 0;
    float *rows = nullptr;                         // [cap_R][V] fp32: one lm_head block
    size_t cap_T = 0;                              // rows of one call the buffers below hold
    uint32_t *targets = nullptr;                   // [cap_T] device
    ScoreRec *recs = nullptr;                      // [cap_T] device
    uint32_t *host_targets = nullptr;              // ... and their pinned images: one copy each way per call
    ScoreRec *host_recs = nullptr;
    int64_t bytes = 0;                             // HBM counted in hbm_bytes
};

struct Shard {
    int device = 0;
    int rank = 0;                // TP rank this shard plays
    hipStream_t stream = nullptr;
    hipStream_t comm_stream = nullptr;   // prefill all-reduces of one token chunk run here while the next chunk computes
    hipEvent_t ev[8] = {};               // e0 e1 (o_proj chunk done) h0 h1 (its all-reduce done) f0 f1 (down done) g0 g1 (reduced)
    int64_t Hs = 0, Hkvs = 0, Is = 0, Ip = 0, Vs = 0, v0 = 0;
    void *embed = nullptr;       // [V,h]
    std::vector<LayerW> layers;
    float *norm = nullptr;
    void *lm_head = nullptr;     // [Vs,h]
    uint8_t *lm_head8 = nullptr; // FL_WEIGHTS_E4M3_ROW: its e4m3 bytes and row scales (lm_head is then the bf16 image)
    float *lm_head_s = nullptr;
    float *cos_tab = nullptr, *sin_tab = nullptr;   // [max_pos][d/2]
    Scratch dec, pre;
    PackedScratch packed;
    ScoreScratch score;
    float *logits_local = nullptr;   // [Vs]
    ArgmaxCand *amax = nullptr;      // [kMaxArgmaxCand] ArgMax candidates left by the decode step's lm_head launch (GemvArgs::amax)
    bool amax_valid = false;         // ... and whether the forward enqueued last produced them (host-side, per enqueue)
    float *logits_full = nullptr;    // [V]
    float *verify_logits = nullptr;  // [kVerifyMaxRows][V] all rows' logits of a verify step (fl_forward_verify); allocated at a model's first one
    uint32_t *verify_out = nullptr;  // [kVerifyWords] its ArgMax ids, accepted count and arrival ticket (launch_verify_select)
    float *verify_scratch = nullptr; // [kVerifyMaxRows][V] the rows' probabilities of a SAMPLED verify step (launch_verify_sample); allocated at a model's first one
    float *verify_adjusted = nullptr; // [kVerifyMaxRows][V] the rule-adjusted, guide-masked rows the selection of a verify step reads (launch_verify_adjust); allocated at the first ruled or guided one
    ScoreRec *verify_recs = nullptr; // [kVerifyMaxRows] the rows' log-prob records of a verify step with log-probs (launch_score_rows); allocated at the first one
    // the persistent decode engine (k_engine.hip): granule edges of one launch and the tag epoch
    unsigned long long *eng_edge[3] = {};   // o_proj deltas [h] | silu(g)*u pairs [Ip/2] | down_proj deltas [h]
    uint32_t *eng_epoch = nullptr;
    std::vector<void *> allocs;
    std::vector<void *> pre_allocs;  // the prefill scratch set: replaced (and freed) when a longer prompt arrives
    int64_t pre_bytes = 0;
    ncclComm_t comm = nullptr;
    PeerComm pc;
};

struct Model {
    std::atomic<int> refs{1};
    std::mutex mu;
    Dims D;
    fl_config cfg_resolved{};
    int dtype = FL_DTYPE_BF16;   // compute dtype
    int tp = 1, tp_mode = FL_TP_NONE;
    bool vocab_parallel = false;
    std::vector<Shard> shards;   // local shards (1 except SINGLE_PROCESS / EMULATED)
    float **emu_ptrs = nullptr;  // EMULATED: device table of per-shard buffers for the local reduce
    float *host_logits = nullptr;   // pinned staging [V]
    uint32_t *host_tokens = nullptr;
    uint32_t *host_verify = nullptr;   // pinned [kVerifyWords]: what a verify step brings back
    ScoreRec *host_verify_recs = nullptr;   // pinned [kVerifyMaxRows]: ... and its log-prob records (fl_forward_verify_lp)
    bool use_graph = true;
    bool fused_decode = true;    // norm / RoPE / KV-append fused into the GEMV kernels
    int decode_weights = FL_WEIGHTS_COMPUTE_DTYPE;   // FL_WEIGHTS_E4M3_ROW: the decode step streams e4m3 weights (k_gemv_w8.hip)
    int engine = -1;             // persistent decode engine (k_engine.hip): 0 off, 1 on, -1 automatic
    int fuse_oproj = 0;          // decode attention + o_proj in one launch (k_attn_oproj.hip): 0 never (default), 1 wherever it fits, -1 where it pays most
    StepState *host_state = nullptr;   // pinned: device step state read back for the error word
    LogprobRec *host_lp = nullptr;     // pinned [kOutTokensCap]: a chunk's log-prob records (allocated at the model's first fl_*_lp call)
    std::vector<ProfRecord> prof;
    bool profiling = false;
    int64_t hbm_bytes = 0;
    size_t esize() const { return dtype == FL_DTYPE_BF16 ? 2 : 4; }
    ~Model();
};

struct CacheShard {
    void *k = nullptr, *v = nullptr;     // [L][Hkvs][max_seq][d]
    StepState *st = nullptr;
    SampleState *ss = nullptr;           // token selection: ArgMax or seeded temperature sampling
    float *sel_scratch = nullptr;        // [V] probabilities / cumulative weights of the sampling path
    uint32_t *out_tokens = nullptr;
    float *part_m = nullptr, *part_l = nullptr, *part_o = nullptr;
    unsigned *counters = nullptr;        // split-S arrival tickets, [Hkvs * q-groups]
    unsigned *heads_done = nullptr;      // [L][Hkv] fused attention+o_proj: split partials published per kv head since set_state
    float *ao_part = nullptr;            // ... and the partials: [Hs][ao_nsplit][d + 4] (o, m, l)
    // the decode step as a graph, one per kind (kStepGuide | kStepRules | kStepLp): [0] is the plain step and never has the launches of the others
    hipGraphExec_t graph[8] = {};
    // token log-probabilities (fl_*_lp): allocated at the cache's first such call, so a cache that never asks pays nothing
    LogprobRec *lp_recs = nullptr;       // [kOutTokensCap] one record per step of a chunk
    LogprobCtl *lp_ctl = nullptr;        // where token_logprobs_kernel finds them, and the call's top_n
    // logit rules (fl_cache_set_logit_rules): allocated at the cache's first install
    LogitRuleEntry *rule_tab = nullptr;  // [V] prompt bit + output count, bias
    LogitRulesCtl *rule_ctl = nullptr;   // the call's scalars and count_input flag, where logit_rules_kernel reads them
    float *logits_adj = nullptr;         // [V] the adjusted row: what token selection reads while rules are installed
    LogitRuleEntry *rule_image = nullptr;   // pinned [V]: the table as an install builds it, source of its one async copy
    // guided decoding (fl_cache_set_guide): allocated at the cache's first install
    GuideCtl *guide_ctl = nullptr;       // the installed guide's arrays and the two state words, where guide_mask_kernel reads them
    float *logits_guided = nullptr;      // [V] the masked row: what token selection reads while a guide is installed
    std::vector<void *> allocs;
};

constexpr size_t kOutTokensCap = 4096;
enum { kStepLp = 1, kStepRules = 2, kStepGuide = 4 };    // kinds of decode step: index into the graph / warm_steps slots

// fl_guide: an immutable token-level automaton of one model in CSR form -- the host copy (the host walks a call's tokens through it:
// it is authoritative for a cache's state) and one device copy, 8 bytes per edge + 8 per state each.  Reference-counted: the creator
// holds one reference, every cache that has it installed another.
struct Guide {
    Model *m = nullptr;
    std::atomic<int> refs{1};
    uint32_t n_states = 0;
    std::vector<uint64_t> row_ptr;
    std::vector<uint32_t> tokens, next;
    uint64_t *row_ptr_dev = nullptr;
    uint32_t *tokens_dev = nullptr, *next_dev = nullptr;
    // the state after selecting token t in state s (no edge: s)
    uint32_t walk(uint32_t s, uint32_t t) const;
    ~Guide();
};

struct Cache {
    Model *m = nullptr;
    size_t max_seq = 0, len = 0;
    size_t seq_alloc = 0;        // max_seq rounded up to 32: row stride of K / column stride of V^T
    bool v_transposed = false;   // bf16 MFMA attention: value cache stored [Hkvs][d][seq_alloc]
    bool rep_attn = false;       // short cache: decode attention replicated inside the o_proj launch (k_attn_rep.hip)
    bool fuse_oproj = false;     // this cache's decode steps use the fused attention+o_proj launch
    int ao_nsplit = 0, ao_waves = 4;   // ... with this many key splits per kv head, 32 * ao_waves keys per split and step
    int nsplit = 1;
    int warm_steps[8] = {};      // eager decode steps done, per kind of step (its graph is captured after the first)
    bool graph_failed = false;
    bool rules_on = false;       // logit rules installed: the steps run logit_rules_kernel and select from logits_adj
    float rule_rp = 1.f, rule_fp = 0.f, rule_pp = 0.f;
    Guide *guide = nullptr;      // guided decoding: the installed automaton (a reference of this cache's own) and the state in which the
    uint32_t guide_state = 0;    // next selected token is looked up -- host state, like len; written to the device per call and chunk
    std::vector<CacheShard> shards;
    ~Cache();
};

// A fixed set of B <= 64 caches of one model decoded together: one read of the weights per step serves every sequence.
// Up to 8 rows the projections are the streaming GEMVs of k_gemv_batch.hip / k_gemv_dma.hip; beyond, the step is the
// prefill-shaped one (rmsnorm_add, short-prompt GEMM, RoPE, attention as launches of their own) at T = B.
// Single GPU, bf16, MFMA-attention shapes.
constexpr int kMaxBatch = 64;
constexpr int kMaxBatchGemv = 8;                 // rows the streaming GEMV kernels hold
struct Batch {
    Model *m = nullptr;
    std::vector<Cache *> caches;
    int B = 0, max_nsplit = 1, nks_o = 1, nks_down = 1;
    bool dma = false;                            // B >= 3: projections on the LDS-DMA ring kernel (k_gemv_dma.hip)
    bool unfused = false;                        // large B: norm / GEMM / RoPE as separate launches around the short-prompt GEMM
    bool plain = false;                          // ... all caches in the plain layout and head_dim 64 / 128: the batch kernels' plain-layout forms (one RoPE and one attention launch per layer)
    bool per_seq = false;                        // fp32 models, caches without the MFMA attention layout: embedding / RoPE / attention as launches per sequence (the single-sequence kernels on row i), the projections still once for all B rows
    Scratch sc;                                  // ... with the prefill scratch layout at T = B
    SeqRef *seqs_dev = nullptr;
    float *x_res = nullptr, *x_res2 = nullptr;   // [B][h]
    float *delta = nullptr;                      // [max(nks_o, nks_down)][B][h]
    void *q = nullptr, *ao = nullptr;            // [B][H*d]
    void *act = nullptr;                         // [B][Ip]
    float *logits = nullptr;                     // [B][V]
    float *logits_local = nullptr, *logits_ranks = nullptr;   // tensor-parallel rank: its [B][Vs] block, and the gathered [tp][B][Vs]
    uint32_t *host_tokens = nullptr;             // pinned [B][kBatchChunk]
    StepState *host_states = nullptr;            // pinned [B]
    hipGraphExec_t graph[8] = {};                // the step per kind (kStepGuide | kStepRules | kStepLp), as a cache's
    bool graph_failed = false;
    int warm_steps[8] = {};
    // fl_batch_decode_each_lp: the step with the log-prob launch behind token selection, the sequences' LogprobCtl pointers [B]
    // (written at the start of every such call) and the pinned [B][kBatchChunk] records; allocated at the batch's first such call
    LogprobCtl **lp_ctls = nullptr;
    LogprobRec *host_lp = nullptr;
    // logit rules: the members' control blocks [B] (null: no rules; written at the start of every decode call with a ruled member and
    // by fl_batch_replace) and the adjusted rows [B][V]; allocated at the batch's first step with a ruled member
    LogitRulesCtl **rule_ctls = nullptr;
    float *logits_adj = nullptr;
    // guided decoding: the same pair -- the members' GuideCtl [B] (null: no guide, the row is copied through) and the masked rows [B][V]
    GuideCtl **guide_ctls = nullptr;
    float *logits_guided = nullptr;
    std::vector<void *> allocs;
    ~Batch();
};
constexpr size_t kBatchChunk = 256;              // decode steps enqueued between two looks at the tokens

int batch_create(Model *m, Cache *const *caches, size_t B, Batch **out);
int batch_replace(Batch *b, size_t slot, Cache *c);     // fl_batch_replace: another stream's cache takes sequence `slot`'s place
// one step for every sequence: tokens[b] at RoPE offset pos[b]; logits_out [B][V] (host) or null
int batch_forward(Batch *b, const uint32_t *tokens, const size_t *pos, float *logits_out, uint32_t *tokens_out);
// n_steps greedy / sampled steps; tokens_out [B][n_steps], n_out [B] (stops counting a sequence at its EOS)
int batch_decode(Batch *b, const uint32_t *first, const size_t *pos, size_t n_steps, int64_t eos,
                 const fl_sampler *sampling, uint32_t *tokens_out, size_t *n_out);
int batch_decode_each(Batch *b, const uint32_t *first, const size_t *pos, size_t n_steps, const int64_t *eos_each,
                      const fl_sampler *sampling_each, uint32_t *tokens_out, size_t *n_out, const fl_logprobs *lp_each = nullptr);

// fl_batch_prefill: n prompts in one forward, sequence i = ids[offsets[i] .. offsets[i+1]) appended to caches[i] at RoPE offset pos[i];
// per sequence the results of forward(m, caches[i], ..); samplers [n] or null (ArgMax), tokens_out [n] / logits_out [n][V] or null
int batch_prefill(Model *m, Cache *const *caches, size_t n, const uint32_t *ids, const size_t *offsets, const size_t *pos,
                  const fl_sampler *samplers, uint32_t *tokens_out, float *logits_out);
// fl_batch_embed: the same pack, the same layers (under opts->mask), and behind them the pooled final hidden states instead of
// lm_head and token selection; out [n][dims] or, FL_POOL_NONE, [offsets[n]][dims].  check_embed: the struct alone plus, where
// h > 0 is known, `dimensions` -- no device needed
int check_embed(const fl_embed *opts, int64_t h);
int batch_embed(Model *m, Cache *const *caches, size_t n, const uint32_t *ids, const size_t *offsets, const size_t *pos,
                const fl_embed *opts, float *out);

int model_create(const fl_config *cfg, const fl_tensor *tensors, size_t n, int compute_dtype,
                 const fl_parallel *par, const fl_model_options *opts, Model **out);
int attn_cache_nsplit(bool v_transposed, size_t max_seq, int64_t d);   // the split count cache_create gives a cache (before FL_ATTN_NSPLIT)
int cache_create(Model *m, size_t max_seq, Cache **out);
// FL_TP_MULTI_PROCESS: export this rank's inbox / map the peers' (handles: tp x FL_IPC_HANDLE_BYTES in rank order)
int comm_ipc_export(Model *m, void *handle_out);
int comm_ipc_connect(Model *m, const void *handles);
bool fused_all_reduce_ready(const Model *m);   // decode all-reduces ride in the GEMV epilogues (comm_ll.h)

// shared by runtime.hip, weights.hip, model.hip, batch.hip and comm.hip
#define FL_NCCL(expr) do { ncclResult_t r_ = (expr); if (r_ != ncclSuccess) { \
    ::fl::set_error("RCCL error %s at %s:%d (%s)", ncclGetErrorString(r_), __FILE__, __LINE__, #expr); \
    return FL_ERR_RCCL; } } while (0)
int env_int(const char *name, int dflt);
int require_device(int *count = nullptr);   // FL_ERR_NO_DEVICE unless a HIP device is visible (*count: how many); sets no device
void debug_inject(const char *site);     // FL_DEBUG_THROW fault injection (tests of the ABI exception barrier)
Launcher make_launcher(Model *m, Shard &sh);
// comm.hip: inbox / LL region of one shard, its table entries, and the group-level steps
int comm_alloc(Model *m, Shard &sh);
void comm_inbox_release(int device, size_t bytes, void *p);   // a destroyed shard's uncached inbox goes to a free list, never back to the runtime (comm.hip)
void comm_forget(void *local);                         // a destroyed shard's inbox leaves the table of handles exported by this process
void comm_set_entry(PeerComm &pc, int r, void *base);
int comm_ll_publish(Model *m, Shard &sh);              // every entry is set: hand the fused all-reduce's table to the device
int comm_connect_loopback(Model *m);                   // TK_DEBUG_TP_LOOPBACK: every entry is this rank's own inbox (timing tool)
int comm_bootstrap_over_rccl(Model *m);                // all-gather the handles through RCCL, connect, self-test, vote
int comm_probe(Model *m, int form, int64_t n, int iters, double *us_per_call);   // fl_comm_probe
int comm_selftest(Model *m, int64_t n, int *ok);                                  // fl_comm_selftest
int comm_check(Model *m);                              // a kernel gave up waiting for a peer -> FL_ERR_RCCL
// n floats in chunks of at most the inbox size; reduce: out = sum over ranks (in == out allowed); gather: out[r * out_stride + i] = in_r[i]
int oneshot(Model *m, Shard &sh, bool gather, const float *in, float *out, int64_t n, int64_t out_stride, hipStream_t on = nullptr);
// mode: 0 = logits to host, 1 = argmax token to host
// device token-selection state for a LogitsProcessor (temperature, top_p, top_k); null: ArgMax.  V: the vocabulary (top_k >= V is
// off), <= 0: unknown.  FL_ERR_BAD_ARGUMENT: wrong struct_size, NaN top_p, negative top_k.
int make_sampler(const fl_sampler *sampling, int64_t V, SampleState *out);
// sampling == null: ArgMax
// lp != null: the chosen tokens' (and top_n most likely tokens') log-probabilities too (fl_*_lp)
int forward(Model *m, Cache *c, const uint32_t *ids, size_t T, size_t pos, float *logits_out, uint32_t *token_out,
            const fl_sampler *sampling = nullptr, const fl_logprobs *lp = nullptr);
int decode_greedy(Model *m, Cache *c, uint32_t first, size_t pos, size_t n_steps, int64_t eos,
                  uint32_t *tokens_out, size_t *n_out, const fl_sampler *sampling = nullptr, const fl_logprobs *lp = nullptr,
                  float *last_row_out = nullptr /* host [V]: the raw row of the last step that ran, copied under the call's lock */);
// fl_forward_score / fl_batch_score (prompt log-probabilities).  check_score: the struct alone plus, where V > 0 is known, the
// targets -- no device needed; the error names the field
int check_score(const fl_score *sc, size_t T, int64_t V);
int forward_score(Model *m, Cache *c, const uint32_t *ids, size_t T, size_t pos, const fl_score *sc);
int batch_score(Model *m, Cache *const *caches, size_t n, const uint32_t *ids, const size_t *offsets, const size_t *pos, const fl_score *sc);
// A forward whose final norm and lm_head run on every row: lm_head in blocks of at most R rows into out ([R][V] fp32), `each`
// enqueued behind every block (rows r0 .. r0 + n of the forward are in out)
struct AllRows {
    float *out;
    int64_t R;
    std::function<int(Launcher &, int64_t r0, int64_t n)> each;
    // never leave a one-row last block where R >= 3 allows it (the block before it gives up a row): a one-row lm_head launch is the
    // planner's T = 1 kernel, another summation order than the rows of every other block see
    bool no_one_row_tail = false;
};
int lm_head_rows(Model *m, Shard &sh, Launcher &L, Scratch &sc, int64_t T, const AllRows &rows);
// the model's [R][V] fp32 block scratch of such a forward (ScoreScratch::rows; R: the score_rows switch now), allocated -- or regrown,
// after waiting for the stream -- by whichever call needs it first: the scoring calls and fl_batch_verify share it
int score_block_scratch(Model *m, Shard &sh, float **rows, int64_t *R);
// One scoring call's rows -> records (shared by the single and the packed path): begin sizes the model's buffers for T rows and
// sends the targets (tg[T], kScoreNoTarget: none); sink() is the AllRows of a forward whose row 0 is row `row0` of the call, one
// score_rows launch (and, with logits_out, one copy of the block) per lm_head block; one() scores a single row another buffer
// holds (a decode step's logits_full); end() -- after the stream was waited for -- scatters the records into the caller's arrays.
struct ScoreCall {
    Model *m; Shard &sh; const fl_score *sc; size_t T;
    int begin(const uint32_t *tg);
    AllRows sink(size_t row0);
    int one(Launcher &L, const float *row, size_t at);
    int fetch();                                   // the records' copy to the pinned buffer, on the stream
    void end();
};
// fl_logprobs: FL_ERR_BAD_ARGUMENT for null, a wrong struct_size, top_n outside 0..FL_LOGPROBS_MAX_TOP (or above V, where V > 0 is
// known), a missing array, nonzero _reserved -- no device needed
int check_logprobs(const fl_logprobs *lp, int64_t V);
// a model that can report log-probs (FL_ERR_UNSUPPORTED under tensor parallelism), and the device / pinned buffers of one cache
int logprobs_supported(const Model *m);
int ensure_logprobs(Model *m, Cache *c);
// record r of a chunk -> row `at` of the caller's arrays
void scatter_logprobs(const LogprobRec &r, const fl_logprobs *lp, size_t at);
// fl_cache_set_logit_rules / fl_cache_logit_counts.  check_logit_rules: the struct and the lists alone (V <= 0: not known), no device
int check_logit_rules(const fl_logit_rules *rules, const uint32_t *prompt_ids, size_t n_prompt, const uint32_t *output_ids, size_t n_output, int64_t V);
int cache_set_logit_rules(Model *m, Cache *c, const fl_logit_rules *rules, const uint32_t *prompt_ids, size_t n_prompt, const uint32_t *output_ids, size_t n_output);
int cache_logit_counts(Model *m, Cache *c, uint32_t *words_out);
// this call's scalars and count_input flag into the cache's control block, on the stream ahead of the call's steps
int set_logit_rules_ctl(Model *m, Cache *c, bool count_input);
// FL_ERR_UNSUPPORTED for an entry point that does not honour a cache's installed rules
int refuse_logit_rules(const Cache *c, const char *what);

// fl_guide_create / fl_guide_destroy / fl_cache_set_guide / fl_cache_guide_state.  check_guide: the struct and the arrays alone
// (V <= 0: not known), no device
int check_guide(const fl_guide_desc *desc, int64_t V);
int guide_create(Model *m, const fl_guide_desc *desc, Guide **out);
void guide_release(Guide *g);
int cache_set_guide(Model *m, Cache *c, Guide *g, uint32_t state);
int cache_guide_state(const Cache *c, uint32_t *state_out);
// the cache's guide arrays and its host state into its control block, on the stream ahead of a call's (or chunk's) steps
int set_guide_ctl(Model *m, Cache *c);
// FL_ERR_UNSUPPORTED for an entry point that does not honour a cache's installed guide
int refuse_guide(const Cache *c, const char *what);

// fl_cache_truncate / fl_forward_verify / fl_decode_lookup (speculative greedy decode)
int cache_truncate(Cache *c, size_t len);
int cache_copy_prefix(Cache *dst, const Cache *src, size_t n);      // fl_cache_copy_prefix (prefix reuse across caches)
int forward_verify(Model *m, Cache *c, uint32_t token, const uint32_t *draft, size_t n_draft, size_t pos, uint32_t *tokens_out,
                   size_t *n_out, float *logits_out, const fl_sampler *sampling = nullptr);
int decode_lookup(Model *m, Cache *c, const uint32_t *corpus, size_t n_corpus, uint32_t first, size_t pos, size_t n_steps, int64_t eos,
                  const fl_lookup *opts, uint32_t *tokens_out, size_t *n_out, fl_spec_stats *stats, const fl_sampler *sampling = nullptr);
// fl_forward_verify_lp / fl_decode_lookup_lp: the same two calls on a cache with logit rules and / or a guide, with log-probs (lp or null)
int forward_verify_lp(Model *m, Cache *c, uint32_t token, const uint32_t *draft, size_t n_draft, size_t pos, const fl_sampler *sampling,
                      const fl_logprobs *lp, uint32_t *tokens_out, size_t *n_out, float *logits_out);
int decode_lookup_lp(Model *m, Cache *c, const uint32_t *corpus, size_t n_corpus, uint32_t first, size_t pos, size_t n_steps, int64_t eos,
                     const fl_lookup *opts, const fl_sampler *sampling, const fl_logprobs *lp, uint32_t *tokens_out, size_t *n_out,
                     fl_spec_stats *stats);
int check_lookup(const fl_lookup *opts);     // FL_ERR_BAD_ARGUMENT: null, wrong struct_size, a range error
// what a verify step may and may not be asked of one cache (sizes, room, tensor parallelism, the sliding window): no device needed
int check_verify(Model *m, Cache *c, size_t n_draft, size_t pos);
// fl_batch_verify / fl_batch_decode_lookup (prefill_packed.hip): the verify steps of n streams as the rows of one packed forward
int batch_verify(Model *m, Cache *const *caches, size_t n, const uint32_t *ids, const size_t *offsets, const size_t *pos,
                 const fl_sampler *samplers, uint32_t *tokens_out, size_t *n_out, float *logits_out);
int batch_decode_lookup(Model *m, Cache *const *caches, size_t n, const uint32_t *corpus, const size_t *corpus_offsets, const uint32_t *first,
                        const size_t *pos, const size_t *n_steps, const int64_t *eos, const fl_lookup *opts, const fl_sampler *samplers,
                        uint32_t *tokens_out, size_t *n_out, fl_spec_stats *stats);

// most K slices (fp32 slabs summed by the next launch) a row-parallel projection may use at T tokens (weights.hip)
constexpr int kMaxKSplit = 4;
constexpr int kMaxKSplitMid = 8;
constexpr int kMidT = 1024;
constexpr int kMaxQkvSplit = 2;   // QKV projection of a long prompt (its grid leaves CUs idle); rope_kv sums the slabs
constexpr int kMaxQkvSplitShort = 4;   // ... of a short prompt / a decode batch (T <= 128: the projection is a weight stream)
int ksplit_cap(int64_t T);
int qkv_split(int64_t T);                    // K slabs a prompt's QKV projection may leave

// shared by weights.hip, model.hip and batch.hip
int dev_alloc(std::vector<void *> &owner, void **p, size_t bytes, int64_t *acct);
int alloc_scratch(Model *m, Shard &sh, Scratch &sc, int64_t T, std::vector<void *> *owner = nullptr);   // owner: who frees the buffers (default: the shard, i.e. at model destruction)
int grow_prefill_scratch(Model *m, Shard &sh, int64_t T);
int check_call(Model *m, Cache *c, size_t T, size_t pos);
int check_token(const Model *m, uint32_t id, const char *what);   // FL_ERR_BAD_ARGUMENT: an id the vocabulary does not have
struct KvLayer {                             // K and V of layer l in one shard of a cache ([L][Hkvs][seq_alloc][d] each)
    void *k, *v;
    KvLayer(const Model *m, const Cache *c, const Shard &sh, const CacheShard &cs, int64_t l) {
        const size_t off = (size_t)l * sh.Hkvs * c->seq_alloc * m->D.d * m->esize();
        k = (char *)cs.k + off; v = (char *)cs.v + off;
    }
};
// decode attention of one cache in the layout it was created with: the MFMA kernel (transposed V) or the plain one
int attend_decode(Launcher &L, const Model *m, const Cache *c, const Shard &sh, const CacheShard &cs, const KvLayer &kv, const void *q, void *ao, const AttnScratch &as);
ResidEpi resid_epi(const Scratch &sc, const Dims &D, const float *next_norm_w);   // residual epilogue of o_proj / down_proj (kernels.h)
// the device StepState (and, ss_set, the token selection) of one cache shard, on the shard's stream
int set_shard_state(Model *m, Shard &sh, CacheShard &cs, uint32_t token, size_t pos, size_t len, size_t call0, uint32_t step, int64_t eos, const SampleState &ss_new, bool ss_set);
// One step as a hipGraph per slot: replay if there is one; after a warm (eager) step capture `enqueue` on every slot's stream,
// instantiate and launch; on any failure destroy what was instantiated, remember it in graph_failed and run eagerly from then on.
struct GraphSlot { int device; hipStream_t stream; hipGraphExec_t *exec; };
int replay_or_capture(const std::vector<GraphSlot> &slots, bool graphable, bool &graph_failed, int &warm_steps, const std::function<int()> &enqueue);

}  // namespace fl
