// runtime.hip -- what the rest of the library stands on: the error text, the reads of the environment, the device check, the CU
// count of the current device and the one table of integer switches (common.h: TuneKey).
#include "model.h"

#include <ctype.h>
#include <stdarg.h>
#include <stdlib.h>

#include <atomic>
#include <mutex>
#include <new>
#include <stdexcept>

namespace fl {

// ------------------------------------------------------------------------------- errors
static thread_local char g_err[1024];
void set_error(const char *fmt, ...) {
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap);
}
const char *last_error() { return g_err; }

// the library's only reads of the environment: the switch table below (integers) and a handful of diagnostic paths / the fault injector (strings)
const char *env_str(const char *name) { const char *s = getenv(name); return s && *s ? s : nullptr; }
int env_int(const char *name, int dflt) { const char *s = env_str(name); return s ? atoi(s) : dflt; }

// ------------------------------------------------------------------------------- the device
int require_device(int *count) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        (void)hipGetLastError();             // the failed query must not stay behind as the thread's sticky error
        FL_FAIL(FL_ERR_NO_DEVICE, "no HIP device visible: this library has no CPU path");
    }
    if (count) *count = n;
    return FL_OK;
}

int device_cu_count() {                      // of the current device (the shards of a group may sit on different ones)
    constexpr int kMaxDevices = 64;
    static std::atomic<int> cached[kMaxDevices];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return 256;
    int n = cached[dev].load();
    if (!n) {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, dev) == hipSuccess) n = p.multiProcessorCount;
        if (n <= 0) n = 256;
        cached[dev].store(n);
    }
    return n;
}

// ------------------------------------------------------------------------------- switches (common.h: TuneKey)
struct TuneEntry { const char *name; int dflt; bool exp_only = false; };   // exp_only: acts in the EXPERIMENTAL build only (Makefile); fl_tune refuses it elsewhere
static const TuneEntry g_tune_table[TK_COUNT] = {
    {"gemm_h4", 1},
    {"gemm_w14", 1},
    {"gemm_rope_4w", 1},
    {"gemm_f32_mfma", 1},
    {"w14_nt", -1},
    {"h4_nt", -1},
    {"h4_split", 0},
    {"h4_pf", 6},
    {"h4_wait_us", 30},
    {"op_maxsplit", 0},
    {"op_linear_dma", 0},
    {"op_hot", 0},
    {"ar_inbox_floats", 131072},
    {"ar_timeout_ms", 20000},
    {"verbose", 0},
    {"tp_fused_ar", 1},
    {"attn_nw", 4},
    {"attn_prefetch", 0, true},
    {"attn_prefetch_lines", 8, true},
    {"attn_prefetch_pct", 100, true},
    {"attn_prefetch_delay", 0, true},
    {"attn_batch_wgs", 256},
    {"attn_pf32_min_t", 0},
    {"attn_pf32_ks2", -1},
    {"attn_pf32_paired", -1},
    {"attn_pf_waves", 0},
    {"attn_pf_stages", 2},
    {"attn_pf_ksplit", 2},
    {"ao_delay", 6, true},
    {"ao_waves", 0, true},
    {"engine_delay", 12, true},
    {"engine_pf", 1, true},
    {"engine_timeout_ms", 2000, true},
    {"sk_minsteps", 8},
    {"gemm_4w", 1},
    {"gemm_groupm", 0},
    {"8p_mink", 8},
    {"gemm_8p", 1},
    {"gemm_256", 1},
    {"gemm_256_split", 1},
    {"gemm_streamk", 1},
    {"gemm_peel", 1},
    {"gemm_resid", 1},
    {"gemm_skinny_maxt", 128},
    {"skinny_stages", 4},
    {"skinny_nt", 1},
    {"skinny_wm", 1},
    {"skinny_loaders", -1, true},
    {"gemm_skinny_maxt2", 256},
    {"gemv_small", 1},
    {"gemv_r", 2},
    {"gemv_u", 0},
    {"batch_u", 0},
    {"batch_mode", 2},
    {"batch_mfma_min", 3},
    {"dma_kt", 128},
    {"force_generic_gemm", 0},
    {"gemm_skinny", 1},
    {"rope_vec", 1},
    {"weight_arena", 1},
    {"ksplit_mid", 0},
    {"prefill_chunk", 8192},
    {"graph", -1},
    {"fused", 1},
    {"allow_any_arch", 0},
    {"engine", 0, true},
    {"fuse_oproj", 0, true},
    {"oneshot", 1},
    {"debug_rccl_self", 0},
    {"attn_mfma", 1},
    {"attn_nsplit", -1},
    {"attn_rep", 1},
    {"sample_walk", 0},
    {"argmax_fused", 1},
    {"tp_overlap", 1},
    {"tp_overlap_min_t", 512},
    {"qkv_split", 8},
    {"tp_graph", 1},
    {"batch_dma_min", 3},
    {"h4_oproj_1k", 1},
    {"h4_tail", 2},
    {"rs_lazy", 1},
    {"batch_unfused_min", -1},
    {"debug_rs_parts", 0},
    {"debug_tp_loopback", 0, true},      // (results are meaningless by design: a timing tool of the EXPERIMENTAL build)
    {"debug_poison", 0},
    {"gemm_skf", 1},
    {"skf_split", 0},
    {"prefill_dma", 1},
    {"oneshot_wide", 1},
    {"f32_rows_max", 64},
    {"gateup_rowsplit", 1},
    {"score_rows", 256},
    {"gemv_resid", 1},
};
static_assert(sizeof(g_tune_table) / sizeof(g_tune_table[0]) == TK_COUNT, "one row per TuneKey, in the enum's order");
static std::atomic<int> g_tune[TK_COUNT];
static std::once_flag g_tune_once;
static void tune_read_env() {
    for (int k = 0; k < TK_COUNT; k++) {
        char env[64] = "FL_";
        size_t n = 3;
        for (const char *c = g_tune_table[k].name; *c && n + 1 < sizeof env; c++) env[n++] = (char)toupper((unsigned char)*c);
        env[n] = 0;
        int v = env_int(env, g_tune_table[k].dflt);
#ifndef FL_EXPERIMENTAL
        if (g_tune_table[k].exp_only) v = g_tune_table[k].dflt;       // the environment cannot reach a kernel that is not compiled in
        if (k == TK_H4_PF) v &= 0xFFFF;
#endif
        g_tune[k].store(v, std::memory_order_relaxed);
    }
}
int tune(TuneKey k) {
    std::call_once(g_tune_once, tune_read_env);
    return g_tune[k].load(std::memory_order_relaxed);
}
void tune_poison_restart();
int tune_set(const char *name, int value) {
    std::call_once(g_tune_once, tune_read_env);
    for (int k = 0; k < TK_COUNT; k++)
        if (!strcmp(name, g_tune_table[k].name)) {
#ifndef FL_EXPERIMENTAL
            if (g_tune_table[k].exp_only) return FL_ERR_UNSUPPORTED;
            if (k == TK_H4_PF) value &= 0xFFFF;      // (bit 16 is a wrong-results timing probe of the experimental build)
#endif
            if (k == TK_DEBUG_POISON) tune_poison_restart();
            g_tune[k].store(value, std::memory_order_relaxed);
            return FL_OK;
        }
    return FL_ERR_BAD_ARGUMENT;
}
void tune_reload_env() {
    std::call_once(g_tune_once, tune_read_env);
    tune_read_env();
}

int raise_dynamic_lds(const void *fn, size_t lds) {
    if (lds < 64 * 1024) return FL_OK;
    static std::mutex mu;
    static std::unordered_map<uint64_t, size_t> raised;           // (function, device) -> bytes granted
    int dev = 0;
    FL_HIP(hipGetDevice(&dev));
    const uint64_t key = (uint64_t)(uintptr_t)fn * 64 + (uint64_t)(dev & 63);
    std::lock_guard<std::mutex> lock(mu);
    auto it = raised.find(key);
    if (it != raised.end() && it->second >= lds) return FL_OK;
    FL_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    raised[key] = lds;
    return FL_OK;
}

// Fault injection for the tests of the ABI's exception barrier: FL_DEBUG_THROW="<site>=<bad_alloc|runtime|int>"
// makes the named site throw, as a failed `new` / std::vector growth would.
void debug_inject(const char *site) {
    const char *s = env_str("FL_DEBUG_THROW");
    if (!s || !*s) return;
    const size_t n = strlen(site);
    if (strncmp(s, site, n) || s[n] != '=') return;
    if (!strcmp(s + n + 1, "bad_alloc")) throw std::bad_alloc();
    if (!strcmp(s + n + 1, "runtime")) throw std::runtime_error("injected failure");
    throw 42;
}

}  // namespace fl
