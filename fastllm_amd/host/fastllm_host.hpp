// fastllm_host.hpp -- host-side mirror of FastLLM's model-trait surface for the causal-LM forward
// path, written in C++ over the C ABI (include/fastllm_mi355x.h).
//
// The reference's host language is Rust and there is no Rust toolchain in the build image, so the
// layer a Rust maintainer would write as `impl ModelInitializer for Mi355xWithConfig`
// (INTEGRATION.md shows that binding) is mirrored here 1:1 in C++: same type names, same argument
// meaning, same error behaviour, so the parity tests read like the reference's own unit tests.
//
//   reference item                                   mirror
//   ------------------------------------------------ -----------------------------------------
//   trait ModelInitializer  (model_initializer.rs:6-22)   static initialize_model / initialize_cache, forward
//   trait ModelArchitecture (model_initializer.rs:24-27)  static get_family / supports_architecture
//   trait ModelCache, CommonCache (cache.rs:5-42)          struct ModelCache, CommonCache
//   BaseModelConfig + ModelConfigValidation (config.rs)    struct BaseModelConfig
//   llama::ConfigFile, LlamaCache, LlamaWithConfig         same names (llama.rs:18-159)
//   mistral::ConfigFile, MistralCache, MistralWithConfig   same names (mistral.rs:16-247)
//   QwenCache, QwenWithConfig                              same names (qwen.rs:13-184)
//   generate_stream / generate_tokens_inner (mod.rs:137-340)   Model<M>::generate_stream_ids (per-stream cache, token callback)
//   Model<M>::generate (mod.rs:363-463)                    Model<M>::generate_ids (token ids in/out;
//                                                          the tokenizer is outside the hot path)
//   trait EmbeddingModel, MiniLMModel (embeddings.rs:17-456)   class EmbeddingModel (embed_ids, embed_batch_ids, compute_similarity_ids)
//
// Errors: anyhow::Result -> fastllm::Error (exception, carries the fl_status code); config
// violations that `assert!`/`expect` in the reference (mistral.rs:109-127, qwen.rs:32-37) throw
// fastllm::Panic.  There is no CPU fallback: Device::Cpu is rejected by initialize_model.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <exception>
#include <functional>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/fastllm_mi355x.h"
#include "guide_compile.hpp"

namespace fastllm {

// ------------------------------------------------------------------------------------ errors
struct Error : std::runtime_error {          // anyhow::Error
    int code;
    Error(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};
struct Panic : std::logic_error {            // assert!/expect in the reference
    explicit Panic(const std::string &m) : std::logic_error(m) {}
};
inline void check(int rc, const char *ctx) {
    if (rc != FL_OK) throw Error(rc, std::string(ctx) + ": " + fl_last_error());
}

// ------------------------------------------------------------------------------------ candle stand-ins
enum class DType { F32 = FL_DTYPE_F32, BF16 = FL_DTYPE_BF16, F16 = FL_DTYPE_F16 };   // candle_core::DType

struct Device {                               // candle_core::Device
    enum Kind { Cpu, Mi355x } kind = Cpu;
    std::vector<int32_t> ordinals;            // one GPU, or the TP group driven by this process
    // load option (no counterpart in the reference): the weight format of the decode step.  FL_WEIGHTS_E4M3_ROW: FP8 weights with one
    // power-of-two scale per row (bf16 compute, one GPU; 1.5x a bf16 model's weight memory) -- initialize_model then goes through
    // fl_model_create_opts, and generate_ids / StreamBatcher run on the FP8 model unchanged
    int32_t decode_weights = FL_WEIGHTS_COMPUTE_DTYPE;
    Device with_decode_weights(fl_weight_format f) const { Device d = *this; d.decode_weights = (int32_t)f; return d; }
    static Device cpu() { return Device{}; }
    static Device mi355x(int ordinal = 0) { Device d; d.kind = Mi355x; d.ordinals = {ordinal}; return d; }
    static Device mi355x_tp(std::vector<int32_t> ords) { Device d; d.kind = Mi355x; d.ordinals = std::move(ords); return d; }
    // main.rs:81-97 on linux: Device::cuda_if_available(0) -> the accelerator when present, else Cpu
    static Device cuda_if_available(int ordinal) {
        int n = 0; fl_device_count(&n);
        return n > ordinal ? mi355x(ordinal) : cpu();
    }
    bool is_cpu() const { return kind == Cpu; }
};

struct Tensor {                               // a borrowed view, like the HashMap<String, Tensor> entries
    DType dtype = DType::F32;
    std::vector<int64_t> shape;
    const void *data = nullptr;
    int32_t device = -1;                      // -1 host
    std::shared_ptr<void> owner;              // keeps host storage alive when the tensor owns it

    static Tensor from_ids(const std::vector<uint32_t> &ids) {          // Tensor::new(ids, dev).reshape((1,T))
        auto buf = std::make_shared<std::vector<uint32_t>>(ids);
        Tensor t; t.dtype = DType::F32; t.shape = {1, (int64_t)ids.size()}; t.data = buf->data(); t.owner = buf;
        return t;
    }
    std::pair<int64_t, int64_t> dims2() const {
        if (shape.size() != 2) throw Error(FL_ERR_SHAPE_MISMATCH, "unexpected rank, expected 2");
        return {shape[0], shape[1]};
    }
    // logits.get(0)?.flatten_all()?.to_vec1::<f32>()  (mod.rs:421; LogitsProcessor::sample)
    const float *f32() const { return static_cast<const float *>(data); }
    int64_t elem_count() const { int64_t n = 1; for (auto s : shape) n *= s; return n; }
};
using TensorMap = std::unordered_map<std::string, Tensor>;

// ------------------------------------------------------------------------------------ cache.rs
struct ModelCache {                           // cache.rs:5-10
    virtual void increment_offset() = 0;
    virtual void reset() = 0;
    virtual size_t get_offset() const = 0;
    virtual ~ModelCache() = default;
};
struct CommonCache : ModelCache {             // cache.rs:13-42
    size_t seqlen_offset = 0;
    void increment_offset() override { seqlen_offset += 1; }
    void reset() override { seqlen_offset = 0; }
    size_t get_offset() const override { return seqlen_offset; }
};

// ------------------------------------------------------------------------------------ minimal JSON (config.json)
namespace detail {
struct JsonFlat {                             // top-level object: numbers, strings, null/bool; nested values skipped
    std::unordered_map<std::string, std::string> raw;
    static void skip_ws(const std::string &s, size_t &i) { while (i < s.size() && std::isspace((unsigned char)s[i])) i++; }
    static std::string parse_string(const std::string &s, size_t &i) {
        std::string out; i++;
        while (i < s.size() && s[i] != '"') { if (s[i] == '\\' && i + 1 < s.size()) i++; out += s[i++]; }
        if (i >= s.size()) throw Error(FL_ERR_BAD_CONFIG, "unterminated string in config JSON");
        i++; return out;
    }
    static void skip_value(const std::string &s, size_t &i) {
        int depth = 0;
        while (i < s.size()) {
            char c = s[i];
            if (c == '"') { parse_string(s, i); continue; }
            if (c == '{' || c == '[') depth++;
            else if (c == '}' || c == ']') { if (depth == 0) return; depth--; }
            else if (c == ',' && depth == 0) return;
            i++;
        }
    }
    explicit JsonFlat(const std::string &s) {
        size_t i = 0; skip_ws(s, i);
        if (i >= s.size() || s[i] != '{') throw Error(FL_ERR_BAD_CONFIG, "config JSON must be an object");
        i++;
        while (true) {
            skip_ws(s, i);
            if (i < s.size() && s[i] == '}') break;
            if (i >= s.size() || s[i] != '"') throw Error(FL_ERR_BAD_CONFIG, "malformed config JSON");
            std::string key = parse_string(s, i);
            skip_ws(s, i);
            if (i >= s.size() || s[i] != ':') throw Error(FL_ERR_BAD_CONFIG, "malformed config JSON (missing ':')");
            i++; skip_ws(s, i);
            size_t b = i;
            if (s[i] == '"') { std::string v = parse_string(s, i); raw[key] = "\"" + v; }
            else { skip_value(s, i); std::string v = s.substr(b, i - b); while (!v.empty() && std::isspace((unsigned char)v.back())) v.pop_back(); raw[key] = v; }
            skip_ws(s, i);
            if (i < s.size() && s[i] == ',') { i++; continue; }
            if (i < s.size() && s[i] == '}') break;
            throw Error(FL_ERR_BAD_CONFIG, "malformed config JSON");
        }
    }
    bool has(const std::string &k) const { auto it = raw.find(k); return it != raw.end() && it->second != "null"; }
    double num(const std::string &k) const {                  // serde: missing non-Option field is an error
        auto it = raw.find(k);
        if (it == raw.end() || it->second == "null") throw Error(FL_ERR_BAD_CONFIG, "missing field `" + k + "`");
        char *end = nullptr; double v = std::strtod(it->second.c_str(), &end);
        if (end == it->second.c_str()) throw Error(FL_ERR_BAD_CONFIG, "invalid type for field `" + k + "`");
        return v;
    }
    std::optional<double> opt(const std::string &k) const { return has(k) ? std::optional<double>(num(k)) : std::nullopt; }
    // serde into usize: a non-negative integer; negative, fractional or out-of-range numbers are a type error, never a cast
    size_t usize(const std::string &k) const {
        const double v = num(k);
        if (!(v >= 0.0) || !(v <= 9007199254740992.0) || (double)(uint64_t)v != v) throw Error(FL_ERR_BAD_CONFIG, "invalid value for field `" + k + "`: expected usize");
        return (size_t)v;
    }
    std::optional<size_t> opt_usize(const std::string &k) const { return has(k) ? std::optional<size_t>(usize(k)) : std::nullopt; }
    std::optional<std::string> str(const std::string &k) const {
        auto it = raw.find(k);
        if (it == raw.end() || it->second.empty() || it->second[0] != '"') return std::nullopt;
        return it->second.substr(1);
    }
};
}  // namespace detail

// ------------------------------------------------------------------------------------ config.rs
struct BaseModelConfig {                      // config.rs:6-18 (also llama::ConfigFile llama.rs:18-29, mistral::ConfigFile mistral.rs:80-92)
    size_t hidden_size = 0, intermediate_size = 0, vocab_size = 0, num_hidden_layers = 0, num_attention_heads = 0;
    std::optional<size_t> num_key_value_heads;
    double rms_norm_eps = 0;
    std::optional<double> rope_theta;
    std::optional<size_t> max_position_embeddings;
    std::optional<size_t> sliding_window;
    std::optional<std::string> torch_dtype;

    static BaseModelConfig from_json(const std::string &text) {          // serde_json::from_str (huggingface.rs:78-79)
        detail::JsonFlat j(text);
        BaseModelConfig c;
        c.hidden_size = j.usize("hidden_size");
        c.intermediate_size = j.usize("intermediate_size");
        c.vocab_size = j.usize("vocab_size");
        c.num_hidden_layers = j.usize("num_hidden_layers");
        c.num_attention_heads = j.usize("num_attention_heads");
        c.num_key_value_heads = j.opt_usize("num_key_value_heads");
        c.rms_norm_eps = j.num("rms_norm_eps");
        c.rope_theta = j.opt("rope_theta");
        c.max_position_embeddings = j.opt_usize("max_position_embeddings");
        c.sliding_window = j.opt_usize("sliding_window");
        c.torch_dtype = j.str("torch_dtype");
        return c;
    }
    // ModelConfigValidation (config.rs:31-54)
    size_t validate_head_dimensions() const {
        if (num_attention_heads == 0) throw Error(FL_ERR_BAD_CONFIG, "hidden_size must be divisible by num_attention_heads");
        size_t head_dim = hidden_size / num_attention_heads;
        if (head_dim * num_attention_heads != hidden_size) throw Error(FL_ERR_BAD_CONFIG, "hidden_size must be divisible by num_attention_heads");
        if (head_dim % 2 != 0) throw Error(FL_ERR_BAD_CONFIG, "head_dim must be even for RoPE embeddings");
        return head_dim;
    }
    void validate_gqa_config() const {
        if (num_key_value_heads && (*num_key_value_heads == 0 || num_attention_heads % *num_key_value_heads != 0))
            throw Error(FL_ERR_BAD_CONFIG, "num_attention_heads must be divisible by num_key_value_heads");
    }
    fl_config to_fl(fl_family family, bool qkv_bias) const {
        fl_config c{};
        c.family = family; c.qkv_bias = qkv_bias;
        c.hidden_size = (int64_t)hidden_size; c.intermediate_size = (int64_t)intermediate_size;
        c.vocab_size = (int64_t)vocab_size; c.num_hidden_layers = (int64_t)num_hidden_layers;
        c.num_attention_heads = (int64_t)num_attention_heads;
        c.num_key_value_heads = (int64_t)num_key_value_heads.value_or(0);
        c.max_position_embeddings = (int64_t)max_position_embeddings.value_or(0);
        c.sliding_window = (int64_t)sliding_window.value_or(0);
        c.rms_norm_eps = rms_norm_eps; c.rope_theta = rope_theta.value_or(0.0);
        return c;
    }
};

// ------------------------------------------------------------------------------------ shared plumbing
namespace detail {
struct ModelHandle {                          // owns one fl_model reference; Clone = refcount bump (mod.rs:155)
    fl_model *m = nullptr;
    explicit ModelHandle(fl_model *mm) : m(mm) {}
    ~ModelHandle() { if (m) fl_model_release(m); }
    ModelHandle(const ModelHandle &) = delete;
};
struct CacheHandle {
    fl_cache *c = nullptr;
    ~CacheHandle() { if (c) fl_cache_destroy(c); }
};

inline size_t default_max_seq(const fl_model *m) {
    fl_model_info info; check(fl_model_get_info(m, &info), "fl_model_get_info");
    size_t cap = 4096;                                         // KV capacity of one request
    if (const char *e = std::getenv("FASTLLM_MAX_SEQ")) cap = (size_t)std::strtoull(e, nullptr, 10);
    return std::min<size_t>(cap, (size_t)info.cfg.max_position_embeddings);
}

inline std::shared_ptr<ModelHandle> create(const fl_config &cfg, const TensorMap &tensors, DType dtype, const Device &device) {
    if (device.is_cpu())
        throw Error(FL_ERR_NO_DEVICE, "the MI355X backend has no CPU path: pass Device::mi355x(..) (main.rs:81-97 picks the accelerator)");
    std::vector<fl_tensor> arr;
    arr.reserve(tensors.size());
    for (auto &kv : tensors) {
        fl_tensor t{};
        t.name = kv.first.c_str(); t.dtype = (int32_t)kv.second.dtype; t.ndim = (int32_t)kv.second.shape.size();
        if (t.ndim > 4) throw Error(FL_ERR_SHAPE_MISMATCH, "tensor " + kv.first + " has rank > 4");
        for (int i = 0; i < t.ndim; i++) t.shape[i] = kv.second.shape[i];
        t.data = kv.second.data; t.device = kv.second.device;
        arr.push_back(t);
    }
    fl_parallel par{};
    par.mode = device.ordinals.size() > 1 ? FL_TP_SINGLE_PROCESS : FL_TP_NONE;
    par.tp_size = (int32_t)std::max<size_t>(1, device.ordinals.size());
    par.device_ids = device.ordinals.data(); par.n_device_ids = (int32_t)device.ordinals.size();
    fl_model *m = nullptr;
    if (device.decode_weights == FL_WEIGHTS_COMPUTE_DTYPE) {
        check(fl_model_create(&cfg, arr.data(), arr.size(), (int32_t)dtype, &par, &m), "Failed to initialize model");
    } else {
        fl_model_options opts{};
        opts.struct_size = (uint32_t)sizeof opts; opts.decode_weights = device.decode_weights;
        check(fl_model_create_opts(&cfg, arr.data(), arr.size(), (int32_t)dtype, &par, &opts, &m), "Failed to initialize model");
    }
    return std::make_shared<ModelHandle>(m);
}

inline Tensor run_forward(fl_model *m, fl_cache *c, const Tensor &input, size_t pos) {
    auto [b, t] = input.dims2();
    if (b != 1) throw Error(FL_ERR_BAD_ARGUMENT, "batch size must be 1 (mod.rs:283-291)");
    fl_model_info info; check(fl_model_get_info(m, &info), "fl_model_get_info");
    auto buf = std::make_shared<std::vector<float>>((size_t)info.cfg.vocab_size);
    check(fl_forward(m, c, static_cast<const uint32_t *>(input.data), (size_t)t, pos, buf->data()), "Model forward pass failed");
    Tensor out; out.dtype = DType::F32; out.data = buf->data(); out.owner = buf;
    return out;
}
}  // namespace detail

enum class PosMode { Reference, Tokens };
// Reference (default): bug-compatible with the reference -- Mistral/Qwen pass a per-call counter as the
// RoPE offset (mistral.rs:226,234; qwen.rs:142-143).  Tokens: the offset is the token position.
inline PosMode pos_mode() {
    const char *e = std::getenv("FASTLLM_POS_MODE");
    return (e && std::string(e) == "tokens") ? PosMode::Tokens : PosMode::Reference;
}

// ------------------------------------------------------------------------------------ llama.rs
struct LlamaCache : ModelCache {              // llama.rs:62-92: wraps candle's Cache{cos,sin,kvs} + an unused counter
    std::shared_ptr<detail::CacheHandle> inner;
    size_t seqlen_offset = 0;
    void increment_offset() override { seqlen_offset += 1; }
    void reset() override { seqlen_offset = 0; }
    size_t get_offset() const override { return seqlen_offset; }
};

struct LlamaWithConfig {
    using Config = BaseModelConfig;           // llama::ConfigFile (llama.rs:18-29): same fields minus sliding_window
    using Cache = LlamaCache;
    std::shared_ptr<detail::ModelHandle> model;

    static std::shared_ptr<detail::ModelHandle> &last() { static std::shared_ptr<detail::ModelHandle> p; return p; }

    // llama.rs:98-123.  From<ConfigFile> (llama.rs:31-50): kv heads default to heads, theta 1e4, max pos 4096.
    static std::pair<LlamaWithConfig, LlamaCache> initialize_model(const Config &config, const TensorMap &tensors, DType dtype, const Device &device) {
        LlamaWithConfig self;
        self.model = detail::create(config.to_fl(FL_FAMILY_LLAMA, false), tensors, dtype, device);
        last() = self.model;
        return {self, new_cache(self.model)};
    }
    // llama.rs:125-145 builds the cache from hard-coded TinyLlama dims because the associated fn cannot see
    // the model (quirk C.2).  Here it is derived from the most recently initialised model of this process
    // (the reference serves one model per process, main.rs:128).
    static LlamaCache initialize_cache(const Device &, DType) {
        if (!last()) throw Error(FL_ERR_BAD_ARGUMENT, "Failed to initialize model cache: no model initialised");
        return new_cache(last());
    }
    // llama.rs:147-149: self.model.forward(input, pos, &mut cache.inner) -- the caller's token position is used
    Tensor forward(const Tensor &input, size_t pos, Cache &cache) const {
        Tensor logits = detail::run_forward(model->m, cache.inner->c, input, pos);
        logits.shape = {1, logits.owner ? (int64_t)static_cast<std::vector<float> *>(logits.owner.get())->size() : 0};   // [1, V] f32
        return logits;
    }
    // the handles and the position bookkeeping the prompt-lookup loop needs (Model<M>::generate_ids with LookupOptions)
    fl_model *raw_model() const { return model->m; }
    fl_cache *raw_cache(Cache &cache) const { return cache.inner->c; }
    void prepare(Cache &) const {}            // (the cache object exists from initialize_cache on)
    size_t rope_offset(size_t pos, const Cache &) const { return pos; }
    void advance(Cache &, size_t) const {}
    static const char *get_family() { return "Llama"; }                                             // llama.rs:153
    static bool supports_architecture(const std::string &a) { return a == "LlamaForCausalLM"; }     // llama.rs:157-159

   private:
    static LlamaCache new_cache(const std::shared_ptr<detail::ModelHandle> &m) {
        LlamaCache c; c.inner = std::make_shared<detail::CacheHandle>();
        check(fl_cache_create(m->m, detail::default_max_seq(m->m), &c.inner->c), "Failed to initialize model cache");
        return c;
    }
};

// ------------------------------------------------------------------------------------ mistral.rs / qwen.rs
// The reference keeps KV inside the candle model (RefCell) and the adapter cache is only a counter
// (mistral.rs:16-47, qwen.rs:59-87).  Here KV is a caller-owned fl_cache attached to the counter object,
// so concurrent streams on one model are sound (quirk C.7).
struct CounterCache : ModelCache {
    size_t seqlen_offset = 0;
    std::shared_ptr<detail::CacheHandle> kv;  // created lazily by forward (initialize_cache cannot see the model)
    void increment_offset() override { seqlen_offset += 1; }
    void reset() override { seqlen_offset = 0; }
    size_t get_offset() const override { return seqlen_offset; }
};
using MistralCache = CounterCache;
using QwenCache = CounterCache;

template <fl_family FAMILY, bool BIAS>
struct CounterFamily {
    using Config = BaseModelConfig;
    using Cache = CounterCache;
    std::shared_ptr<detail::ModelHandle> model;

    static size_t get_head_dim(size_t hidden_size, size_t num_attention_heads) {                    // mistral.rs:67-76
        if (num_attention_heads == 0 || (hidden_size / num_attention_heads) * num_attention_heads != hidden_size)
            throw Panic("hidden_size must be divisible by num_attention_heads");
        return hidden_size / num_attention_heads;
    }
    static void validate(const Config &cf) {                                                        // mistral.rs:93-127, qwen.rs:30-37
        size_t head_dim = get_head_dim(cf.hidden_size, cf.num_attention_heads);
        size_t kv = cf.num_key_value_heads.value_or(cf.num_attention_heads);
        if (kv == 0 || cf.num_attention_heads % kv != 0) throw Panic("num_attention_heads must be divisible by num_key_value_heads");
        if (head_dim % 2 != 0) throw Panic("head_dim must be even for RoPE embeddings");
    }
    static std::pair<CounterFamily, Cache> initialize_model(const Config &config, const TensorMap &tensors, DType dtype, const Device &device) {
        validate(config);
        CounterFamily self;
        self.model = detail::create(config.to_fl(FAMILY, BIAS), tensors, dtype, device);
        return {self, Cache{}};
    }
    static Cache initialize_cache(const Device &, DType) { return Cache{}; }                        // mistral.rs:202-204, qwen.rs:119-121
    // mistral.rs:206-236 / qwen.rs:123-151: `_pos` is ignored; offset 0 clears the KV cache; the model is run
    // at the per-call counter; the counter then advances by ONE per call (quirk C.1).
    Tensor forward(const Tensor &input, size_t pos, Cache &cache) const {
        if (!cache.kv) {
            cache.kv = std::make_shared<detail::CacheHandle>();
            check(fl_cache_create(model->m, detail::default_max_seq(model->m), &cache.kv->c), "Failed to initialize model cache");
        }
        if (cache.seqlen_offset == 0) fl_cache_reset(cache.kv->c);                                  // clear_kv_cache()
        const size_t rope_offset = pos_mode() == PosMode::Reference ? cache.seqlen_offset : pos;
        Tensor logits = detail::run_forward(model->m, cache.kv->c, input, rope_offset);
        logits.shape = {1, 1, (int64_t)static_cast<std::vector<float> *>(logits.owner.get())->size()};   // [1,1,V]
        cache.increment_offset();
        return logits;
    }
    // the prompt-lookup loop (Model<M>::generate_ids with LookupOptions): the cache exists after the prompt's forward; a verify step
    // of n rows stands for n calls of `forward`, so the per-call counter (quirk C.1) advances by n and row t runs at counter + t
    fl_model *raw_model() const { return model->m; }
    fl_cache *raw_cache(Cache &cache) const { return cache.kv->c; }
    // what `forward` does ahead of its run, for a caller that makes the prompt's call itself (generate_ids with log-probs)
    void prepare(Cache &cache) const {
        if (!cache.kv) {
            cache.kv = std::make_shared<detail::CacheHandle>();
            check(fl_cache_create(model->m, detail::default_max_seq(model->m), &cache.kv->c), "Failed to initialize model cache");
        }
        if (cache.seqlen_offset == 0) fl_cache_reset(cache.kv->c);
    }
    size_t rope_offset(size_t pos, const Cache &cache) const { return pos_mode() == PosMode::Reference ? cache.seqlen_offset : pos; }
    void advance(Cache &cache, size_t calls) const { cache.seqlen_offset += calls; }
};

struct MistralWithConfig : CounterFamily<FL_FAMILY_MISTRAL, false> {
    MistralWithConfig() = default;
    MistralWithConfig(const CounterFamily &b) : CounterFamily(b) {}
    static std::pair<MistralWithConfig, MistralCache> initialize_model(const Config &c, const TensorMap &t, DType d, const Device &dev) {
        auto r = CounterFamily::initialize_model(c, t, d, dev); return {MistralWithConfig(r.first), r.second};
    }
    static const char *get_family() { return "Mistral"; }                                           // mistral.rs:240
    static bool supports_architecture(const std::string &a) { return a == "MistralForCausalLM"; }   // mistral.rs:244-246
};

struct QwenWithConfig : CounterFamily<FL_FAMILY_QWEN2, true> {
    QwenWithConfig() = default;
    QwenWithConfig(const CounterFamily &b) : CounterFamily(b) {}
    // qwen.rs:30-37: validate_head_dimensions().expect(..) / validate_gqa_config().expect(..) -> panic
    static std::pair<QwenWithConfig, QwenCache> initialize_model(const Config &c, const TensorMap &t, DType d, const Device &dev) {
        try { c.validate_head_dimensions(); } catch (const Error &e) { throw Panic(std::string("Invalid head dimensions: ") + e.what()); }
        try { c.validate_gqa_config(); } catch (const Error &e) { throw Panic(std::string("Invalid GQA configuration: ") + e.what()); }
        auto r = CounterFamily::initialize_model(c, t, d, dev); return {QwenWithConfig(r.first), r.second};
    }
    static const char *get_family() { return "Qwen"; }                                              // qwen.rs:174
    static bool supports_architecture(const std::string &a) {                                       // qwen.rs:178-183
        return a == "Qwen2ForCausalLM" || a == "Qwen2_5_VLForConditionalGeneration";
    }
};

// ------------------------------------------------------------------------------------ mod.rs: Model<M>
inline uint32_t argmax_last(const float *v, size_t n) {      // LogitsProcessor ArgMax: max_by(total_cmp) -> last max
    size_t best = 0;
    for (size_t i = 1; i < n; i++) if (!(v[i] < v[best])) best = i;
    return (uint32_t)best;
}

// rand 0.8 `StdRng` as LogitsProcessor seeds it: ChaCha12, key = SeedableRng::seed_from_u64 (PCG32 XSH-RR
// expansion of the u64 into eight little-endian words), 64-bit block counter from 0, stream id 0, consumed
// one u32 word at a time.
class StdRng {
   public:
    explicit StdRng(uint64_t seed) {
        uint64_t st = seed;
        for (auto &k : key_) {
            st = st * 6364136223846793005ull + 11634580027462260723ull;
            const uint32_t xs = (uint32_t)(((st >> 18) ^ st) >> 27), rot = (uint32_t)(st >> 59);
            k = (xs >> rot) | (xs << ((32 - rot) & 31));
        }
    }
    uint32_t next_u32() {
        if ((word_ & 15) == 0) block(word_ >> 4);
        return buf_[word_++ & 15];
    }
    uint64_t words_consumed() const { return word_; }

   private:
    static uint32_t rotl(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }
    static void qr(uint32_t &a, uint32_t &b, uint32_t &c, uint32_t &d) {
        a += b; d ^= a; d = rotl(d, 16); c += d; b ^= c; b = rotl(b, 12);
        a += b; d ^= a; d = rotl(d, 8);  c += d; b ^= c; b = rotl(b, 7);
    }
    void block(uint64_t counter) {
        uint32_t s[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u};
        for (int i = 0; i < 8; i++) s[4 + i] = key_[i];
        s[12] = (uint32_t)counter; s[13] = (uint32_t)(counter >> 32); s[14] = s[15] = 0;
        uint32_t x[16];
        std::memcpy(x, s, sizeof x);
        for (int r = 0; r < 12; r += 2) {
            qr(x[0], x[4], x[8], x[12]); qr(x[1], x[5], x[9], x[13]); qr(x[2], x[6], x[10], x[14]); qr(x[3], x[7], x[11], x[15]);
            qr(x[0], x[5], x[10], x[15]); qr(x[1], x[6], x[11], x[12]); qr(x[2], x[7], x[8], x[13]); qr(x[3], x[4], x[9], x[14]);
        }
        for (int i = 0; i < 16; i++) buf_[i] = x[i] + s[i];
    }
    uint32_t key_[8], buf_[16];
    uint64_t word_ = 0;
};

// candle_transformers::generation::LogitsProcessor as the reference builds it:
// LogitsProcessor::new(Default::default(), Some(temperature as f64), None) (mod.rs:157-158,373-374).
// This is the reference's own host-side shape (logits on the host, mod.rs:421-428); the device-side
// equivalent is fl_forward_sample / fl_decode_sample.
//
// With top_p / top_k it is LogitsProcessor::from_sampling(seed, Sampling::TopP / TopK / TopKThenTopP) [UPSTREAM-RECALLED], with the
// semantics of fl_sampler (include/fastllm_mi355x.h): the kept set is a prefix of the order by prs descending, the LOWER index first
// among equals; top_p (0 < top_p < 1, compared as f32) ends it where the sequential f32 running sum is no longer < top_p, top_k
// (0 < top_k < n) at rank top_k; the draw runs over the masked vector in vocabulary order.  top_k = 1 keeps the LOWEST maximal
// index; ArgMax (temperature < 1e-7, whatever the other two say) keeps the LAST.  The device-side equivalent is fl_*_sample_ex.
class LogitsProcessor {
   public:
    LogitsProcessor(uint64_t seed, std::optional<double> temperature, std::optional<double> top_p = std::nullopt,
                    std::optional<size_t> top_k = std::nullopt) : rng_(seed) {
        if (temperature && !(*temperature < 1e-7)) { sampling_ = true; temperature_ = *temperature; }
        if (top_p && *top_p != *top_p) throw Error(FL_ERR_BAD_ARGUMENT, "top_p is NaN");
        if (top_p && *top_p > 0.0 && *top_p < 1.0) { top_p_on_ = true; top_p_ = (float)*top_p; }
        if (top_k) top_k_ = *top_k;                                   // 0 or >= n: off
    }
    bool is_argmax() const { return !sampling_; }
    size_t kept() const { return kept_; }                             // tokens the last sample() kept (n without a filter)
    // the filter and the draw alone, on probabilities the caller computed (tests)
    uint32_t sample_prs(const float *prs, size_t n) {
        if (n == 0) throw Error(FL_ERR_BAD_ARGUMENT, "empty logits");
        prs_.assign(prs, prs + n);
        return draw(n);
    }
    double temperature() const { return temperature_; }
    uint64_t draws() const { return rng_.words_consumed(); }
    uint32_t sample(const float *logits, size_t n) {
        if (n == 0) throw Error(FL_ERR_BAD_ARGUMENT, "empty logits");
        if (!sampling_) return argmax_last(logits, n);
        // prs = softmax_last_dim(logits / temperature): `Tensor / f64` is affine(1/t, 0) in the tensor's dtype
        const float mul = (float)(1.0 / temperature_);
        prs_.resize(n);
        float mx = -INFINITY;
        for (size_t i = 0; i < n; i++) { prs_[i] = logits[i] * mul; if (prs_[i] > mx) mx = prs_[i]; }
        float sum = 0.f;
        for (size_t i = 0; i < n; i++) { prs_[i] = std::exp(prs_[i] - mx); sum += prs_[i]; }
        for (size_t i = 0; i < n; i++) prs_[i] /= sum;
        return draw(n);
    }

   private:
    // Sampling::TopP / TopK / TopKThenTopP: zero everything outside the kept prefix of the sorted order
    void filter(size_t n) {
        kept_ = n;
        const bool k_on = top_k_ > 0 && top_k_ < n;
        if (!top_p_on_ && !k_on) return;
        order_.resize(n);
        for (size_t i = 0; i < n; i++) order_[i] = (uint32_t)i;
        std::stable_sort(order_.begin(), order_.end(), [&](uint32_t a, uint32_t b) { return prs_[a] > prs_[b]; });
        size_t m = n;
        if (top_p_on_) {
            float cum = 0.f;
            for (size_t j = 0; j < n; j++) {
                volatile float c = cum + prs_[order_[j]];              // sequential f32, never widened
                cum = c;
                if (!(cum < top_p_)) { m = j + 1; break; }
            }
        }
        if (k_on) m = std::min(m, top_k_);
        for (size_t j = m; j < n; j++) prs_[order_[j]] = 0.f;
        kept_ = m;
    }
    uint32_t draw(size_t n) {
        filter(n);
        // WeightedIndex::new: running f32 total, left to right; weights must be >= 0 and not all zero
        float total = 0.f;
        for (size_t i = 0; i < n; i++) {
            if (!(prs_[i] >= 0.f)) throw Error(FL_ERR_BAD_ARGUMENT, "Failed to sample next token: invalid weight");
            total = i == 0 ? prs_[0] : total + prs_[i];
        }
        if (total == 0.f) throw Error(FL_ERR_BAD_ARGUMENT, "Failed to sample next token: all weights zero");
        // UniformFloat::<f32>::new(0, total) and one sample
        float scale = total;
        const float max_rand = 1.0f - 1.1920929e-07f;
        while (mul_rn(scale, max_rand) >= total) { uint32_t b; std::memcpy(&b, &scale, 4); b -= 1; std::memcpy(&scale, &b, 4); }
        const uint32_t bits = (rng_.next_u32() >> 9) | 0x3f800000u;
        float v12; std::memcpy(&v12, &bits, 4);
        const float chosen = mul_rn(v12 - 1.0f, scale);
        // partition_point(|w| w <= chosen) over the n-1 cumulative weights
        float cum = prs_[0];
        size_t idx = 0;
        while (idx < n - 1 && cum <= chosen) { idx++; cum += prs_[idx]; }
        return (uint32_t)idx;
    }
    static float mul_rn(float a, float b) { volatile float r = a * b; return r; }     // a product, never fused with an add
    StdRng rng_;
    bool sampling_ = false;
    double temperature_ = 0;
    bool top_p_on_ = false;
    float top_p_ = 0.f;
    size_t top_k_ = 0, kept_ = 0;
    std::vector<float> prs_;
    std::vector<uint32_t> order_;
};

// a request's sampling beyond its temperature (chat.rs would carry them as request.top_p / request.top_k); both empty: Sampling::All
struct SamplingOptions {
    std::optional<double> top_p;
    std::optional<size_t> top_k;
    fl_sampler to_ffi(double temperature, uint64_t draws_done) const {
        fl_sampler s{};
        s.struct_size = (uint32_t)sizeof(fl_sampler);
        s.temperature = temperature; s.seed = 0; s.draws_done = draws_done;
        s.top_p = top_p ? *top_p : 0.0;
        s.top_k = top_k ? (int32_t)std::min<size_t>(*top_k, (size_t)INT32_MAX) : 0;
        return s;
    }
};

// Per emitted token its log-probability and, row-major [n][top_n], the ids and log-probabilities of the top_n most likely tokens of
// its step (generate_ids with top_logprobs): log-softmax of the model's own logits -- temperature 1, nothing masked -- computed on the
// device (fl_*_lp), whatever sampler chose the token.  New capability; the reference reports none.
struct TokenLogprobs {
    std::vector<float> token;
    std::vector<uint32_t> top_ids;
    std::vector<float> top;
    int top_n = 0;
};

// Prompt log-probabilities (score_ids): per row of a scored forward the log-probability of the NEXT id of the text (NaN for the last
// row, which has none), its rank in the order "logit descending, lower index first" (1 = the most likely id; 0: none) and, row-major
// [n][top_n], the most likely ids and theirs -- TokenLogprobs' shape with ranks.  Computed on the device (fl_forward_score) from the
// model's own distribution.  New capability; the reference reports none.
struct ScoredTokens {
    std::vector<float> token;
    std::vector<uint32_t> rank;
    std::vector<uint32_t> top_ids;
    std::vector<float> top;
    int top_n = 0;
};

// A request's logit_bias and repetition / frequency / presence penalties (fl_logit_rules): installed on the request's cache, applied
// on the device to every row a token is selected from, the output counts kept by the decode loop itself.  New capability; the
// reference has none.  repetition_penalty 1 and the other two 0 are off; a bias of -inf bans an id.
struct LogitRules {
    std::vector<std::pair<uint32_t, float>> logit_bias;
    float repetition_penalty = 1.f, frequency_penalty = 0.f, presence_penalty = 0.f;
    // on cache `c`: prompt marks its ids as seen, output seeds the counts (a request that resumes)
    void install(fl_model *m, fl_cache *c, const std::vector<uint32_t> &prompt, const std::vector<uint32_t> &output = {}) const {
        std::vector<uint32_t> ids; std::vector<float> values;
        for (auto &b : logit_bias) { ids.push_back(b.first); values.push_back(b.second); }
        fl_logit_rules r{};
        r.struct_size = (uint32_t)sizeof(fl_logit_rules);
        r.n_bias = (uint32_t)ids.size(); r.bias_ids = ids.empty() ? nullptr : ids.data(); r.bias_values = values.empty() ? nullptr : values.data();
        r.repetition_penalty = repetition_penalty; r.frequency_penalty = frequency_penalty; r.presence_penalty = presence_penalty;
        check(fl_cache_set_logit_rules(m, c, &r, prompt.empty() ? nullptr : prompt.data(), prompt.size(), output.empty() ? nullptr : output.data(), output.size()),
              "fl_cache_set_logit_rules");
    }
    static void remove(fl_model *m, fl_cache *c) { check(fl_cache_set_logit_rules(m, c, nullptr, nullptr, 0, nullptr, 0), "fl_cache_set_logit_rules"); }
};

// Guided decoding (fl_guide): a token-level automaton -- what compile_guide (guide_compile.hpp) makes of a grammar compiler's byte
// DFA, or any index over token ids -- on the device, shared by every request that uses the same response format.  New capability; the
// reference has none.  The handle is reference-counted: copies share one fl_guide, and a cache that has it installed keeps it alive.
class Guide {
  public:
    Guide() = default;
    Guide(fl_model *m, const std::vector<uint64_t> &row_ptr, const std::vector<uint32_t> &tokens, const std::vector<uint32_t> &next) {
        if (row_ptr.empty() || tokens.size() != next.size() || row_ptr.back() != tokens.size())
            throw Error(FL_ERR_BAD_ARGUMENT, "Guide: row_ptr, tokens and next do not describe one CSR");
        fl_guide_desc d{};
        d.struct_size = (uint32_t)sizeof(fl_guide_desc);
        d.n_states = (uint32_t)(row_ptr.size() - 1);
        d.row_ptr = row_ptr.data(); d.tokens = tokens.data(); d.next = next.data();
        fl_guide *g = nullptr;
        check(fl_guide_create(m, &d, &g), "fl_guide_create");
        g_ = std::shared_ptr<fl_guide>(g, [](fl_guide *x) { fl_guide_destroy(x); });
    }
    Guide(fl_model *m, const GuideTable &t) : Guide(m, t.row_ptr, t.tokens, t.next) {}
    fl_guide *raw() const { return g_.get(); }
    explicit operator bool() const { return (bool)g_; }

  private:
    std::shared_ptr<fl_guide> g_;
};
// A request's guide and the state its first token is selected in (GuideTable::start_state).
struct GuideOptions {
    Guide guide;
    uint32_t start_state = 0;
    void install(fl_model *m, fl_cache *c) const {
        if (!guide) throw Error(FL_ERR_BAD_ARGUMENT, "GuideOptions: no guide");
        check(fl_cache_set_guide(m, c, guide.raw(), start_state), "fl_cache_set_guide");
    }
    static void remove(fl_model *m, fl_cache *c) { check(fl_cache_set_guide(m, c, nullptr, 0), "fl_cache_set_guide"); }
};

// Prompt-lookup drafting for greedy requests (fl_lookup): the continuation that followed the most recent earlier occurrence of the
// current n-gram is verified in one forward (fl_forward_verify).  New capability; the tokens are those of the plain greedy loop.
struct LookupOptions {
    int max_draft = 7, ngram_max = 3, ngram_min = 1;
    fl_lookup to_ffi() const {
        fl_lookup o{};
        o.struct_size = (uint32_t)sizeof(fl_lookup);
        o.max_draft = max_draft; o.ngram_max = ngram_max; o.ngram_min = ngram_min;
        return o;
    }
};
inline void require_greedy(float temperature) {
    if (!(temperature < 1e-7))
        throw Error(FL_ERR_UNSUPPORTED, "prompt-lookup decoding is greedy only: temperature must be below 1e-7 (speculative sampling would change "
                                        "how the seeded stream is consumed)");
}

template <class M>
struct Model {                                // mod.rs:342-361
    M model;
    Device device;
    typename M::Cache cache;
    DType dtype = DType::BF16;                // mod.rs:359
    size_t forwards = 0;                      // forwards executed by the last generate (incl. the wasted one, C.5)

    Model(M m, Device d, typename M::Cache c) : model(std::move(m)), device(std::move(d)), cache(std::move(c)) {}

    // Model::generate (mod.rs:363-463) on token ids.  eos = tokenizer.token_to_id("</s>") (mod.rs:431).
    std::vector<uint32_t> generate_ids(const std::vector<uint32_t> &prompt, size_t max_tokens, float temperature,
                                       std::optional<uint32_t> eos = std::nullopt) {
        return generate_ids(prompt, max_tokens, temperature, eos, SamplingOptions{});
    }
    // ... with top_p / top_k (LogitsProcessor::new(seed, Some(temperature), top_p) / from_sampling)
    std::vector<uint32_t> generate_ids(const std::vector<uint32_t> &prompt, size_t max_tokens, float temperature,
                                       std::optional<uint32_t> eos, const SamplingOptions &opt) {
        cache = M::initialize_cache(device, dtype);                       // mod.rs:370
        LogitsProcessor logits_processor(0, (double)temperature, opt.top_p, opt.top_k);   // mod.rs:373-374 (Default::default() seed)
        if (prompt.empty()) throw Error(FL_ERR_BAD_ARGUMENT, "Tokenization error: empty prompt");
        Tensor input = Tensor::from_ids(prompt);                           // mod.rs:386-394
        std::vector<uint32_t> output_ids;
        size_t pos = 0;
        forwards = 0;
        Tensor logits = model.forward(input, pos, cache); forwards++;      // mod.rs:402-405
        pos += prompt.size();                                              // mod.rs:408
        for (size_t i = 0; i < max_tokens; i++) {                          // mod.rs:411
            const uint32_t next = logits_processor.sample(logits.f32(), (size_t)logits.elem_count());   // mod.rs:421-428
            if (eos && next == *eos) break;                                // mod.rs:431-436
            output_ids.push_back(next);                                    // mod.rs:438
            Tensor next_input = Tensor::from_ids({next});                  // mod.rs:441-444
            logits = model.forward(next_input, pos, cache); forwards++;    // mod.rs:446-451 (also after the last token)
            pos += 1;                                                      // mod.rs:452
        }
        return output_ids;
    }

    // ... with log-probabilities (0 <= top_logprobs <= FL_LOGPROBS_MAX_TOP): token selection stays on the device -- the first token
    // from fl_forward_sample_lp on the prompt, the other max_tokens - 1 from fl_decode_sample_lp -- so the ids are those of the
    // overload above (the device sampler is the host LogitsProcessor bit for bit) and `out` holds one record per id.  `forwards`
    // counts the prompt's forward and the decode steps; the reference's wasted forward behind the last token (C.5) is not run.
    std::vector<uint32_t> generate_ids(const std::vector<uint32_t> &prompt, size_t max_tokens, float temperature,
                                       std::optional<uint32_t> eos, const SamplingOptions &opt, int top_logprobs, TokenLogprobs *out) {
        if (!out) throw Error(FL_ERR_BAD_ARGUMENT, "generate_ids: null TokenLogprobs");
        if (top_logprobs < 0 || top_logprobs > FL_LOGPROBS_MAX_TOP) throw Error(FL_ERR_BAD_ARGUMENT, "generate_ids: top_logprobs out of range");
        cache = M::initialize_cache(device, dtype);
        if (prompt.empty()) throw Error(FL_ERR_BAD_ARGUMENT, "Tokenization error: empty prompt");
        *out = TokenLogprobs{};
        out->top_n = top_logprobs;
        forwards = 0;
        std::vector<uint32_t> output_ids;
        if (max_tokens == 0) { model.forward(Tensor::from_ids(prompt), 0, cache); forwards++; return output_ids; }
        const size_t w = (size_t)top_logprobs;
        output_ids.assign(max_tokens, 0);
        out->token.assign(max_tokens, 0.f);
        out->top_ids.assign(max_tokens * w, 0);
        out->top.assign(max_tokens * w, 0.f);
        auto lp_at = [&](size_t row) {
            fl_logprobs lp{};
            lp.struct_size = (uint32_t)sizeof(fl_logprobs);
            lp.top_n = top_logprobs;
            lp.token_logprob = out->token.data() + row;
            lp.top_ids = w ? out->top_ids.data() + row * w : nullptr;
            lp.top_logprobs = w ? out->top.data() + row * w : nullptr;
            return lp;
        };
        model.prepare(cache);
        fl_cache *c = model.raw_cache(cache);
        const fl_sampler s0 = opt.to_ffi((double)temperature, 0);
        const fl_logprobs lp0 = lp_at(0);
        check(fl_forward_sample_lp(model.raw_model(), c, prompt.data(), prompt.size(), model.rope_offset(0, cache), &s0, &output_ids[0], &lp0),
              "Model forward pass failed");
        model.advance(cache, 1); forwards++;
        size_t n = 0;
        const bool ended = eos && output_ids[0] == *eos;
        if (!ended && max_tokens > 1) {
            const fl_sampler s1 = opt.to_ffi((double)temperature, 1);
            const fl_logprobs lp1 = lp_at(1);
            const size_t len0 = fl_cache_len(c);
            check(fl_decode_sample_lp(model.raw_model(), c, output_ids[0], model.rope_offset(prompt.size(), cache), max_tokens - 1,
                                      eos ? (int64_t)*eos : -1, &s1, output_ids.data() + 1, &n, &lp1), "Model forward pass failed");
            model.advance(cache, fl_cache_len(c) - len0);
            forwards += fl_cache_len(c) - len0;
        }
        const size_t total = ended ? 0 : 1 + n;
        output_ids.resize(total); out->token.resize(total); out->top_ids.resize(total * w); out->top.resize(total * w);
        return output_ids;
    }

    // What an `echo` + `logprobs` request, a `loglikelihood` evaluation or a reranker asks for: every id of a text scored under the
    // model, from a fresh cache, in ONE forward (fl_forward_score) -- row i against ids[i + 1].  The cache afterwards is the one a
    // forward of the ids leaves.
    ScoredTokens score_ids(const std::vector<uint32_t> &ids, int top_logprobs) {
        if (top_logprobs < 0 || top_logprobs > FL_LOGPROBS_MAX_TOP) throw Error(FL_ERR_BAD_ARGUMENT, "score_ids: top_logprobs out of range");
        cache = M::initialize_cache(device, dtype);
        if (ids.empty()) throw Error(FL_ERR_BAD_ARGUMENT, "Tokenization error: empty prompt");
        ScoredTokens out;
        out.top_n = top_logprobs;
        const size_t w = (size_t)top_logprobs, n = ids.size();
        out.token.assign(n, 0.f); out.rank.assign(n, 0); out.top_ids.assign(n * w, 0); out.top.assign(n * w, 0.f);
        fl_score sc{};
        sc.struct_size = (uint32_t)sizeof(fl_score);
        sc.top_n = top_logprobs;
        sc.target_logprob = out.token.data();
        sc.target_rank = out.rank.data();
        sc.top_ids = w ? out.top_ids.data() : nullptr;
        sc.top_logprobs = w ? out.top.data() : nullptr;
        model.prepare(cache);
        check(fl_forward_score(model.raw_model(), model.raw_cache(cache), ids.data(), n, model.rope_offset(0, cache), &sc), "Model forward pass failed");
        model.advance(cache, 1);                                          // (one forward call, as behind the prompt in generate_ids)
        forwards = 1;
        return out;
    }

    // ... with logit rules: installed on the fresh cache (the prompt's ids marked as seen) before the first fl_forward_sample_ex, so
    // the first token is already selected from the adjusted row; the other max_tokens - 1 come from fl_decode_sample_ex, which counts
    // every token it is fed.  Token selection stays on the device throughout.  `forwards` as in the log-prob overload.
    std::vector<uint32_t> generate_ids(const std::vector<uint32_t> &prompt, size_t max_tokens, float temperature,
                                       std::optional<uint32_t> eos, const SamplingOptions &opt, const LogitRules &rules) {
        return generate_ids(prompt, max_tokens, temperature, eos, opt, &rules, nullptr);
    }
    // ... with a guide (and optionally rules beside it: rules first, mask last): installed on the fresh cache at its start state, so
    // the first token is already selected among the ids the automaton allows; the library advances the state with every token.
    std::vector<uint32_t> generate_ids(const std::vector<uint32_t> &prompt, size_t max_tokens, float temperature,
                                       std::optional<uint32_t> eos, const SamplingOptions &opt, const GuideOptions &guide,
                                       const LogitRules *rules = nullptr) {
        return generate_ids(prompt, max_tokens, temperature, eos, opt, rules, &guide);
    }
    std::vector<uint32_t> generate_ids(const std::vector<uint32_t> &prompt, size_t max_tokens, float temperature,
                                       std::optional<uint32_t> eos, const SamplingOptions &opt, const LogitRules *rules, const GuideOptions *guide) {
        cache = M::initialize_cache(device, dtype);
        if (prompt.empty()) throw Error(FL_ERR_BAD_ARGUMENT, "Tokenization error: empty prompt");
        forwards = 0;
        std::vector<uint32_t> output_ids;
        if (max_tokens == 0) { model.forward(Tensor::from_ids(prompt), 0, cache); forwards++; return output_ids; }
        output_ids.assign(max_tokens, 0);
        model.prepare(cache);
        fl_cache *c = model.raw_cache(cache);
        if (rules) rules->install(model.raw_model(), c, prompt);
        if (guide) guide->install(model.raw_model(), c);
        const fl_sampler s0 = opt.to_ffi((double)temperature, 0);
        check(fl_forward_sample_ex(model.raw_model(), c, prompt.data(), prompt.size(), model.rope_offset(0, cache), &s0, &output_ids[0]),
              "Model forward pass failed");
        model.advance(cache, 1); forwards++;
        size_t n = 0;
        const bool ended = eos && output_ids[0] == *eos;
        if (!ended && max_tokens > 1) {
            const fl_sampler s1 = opt.to_ffi((double)temperature, 1);
            const size_t len0 = fl_cache_len(c);
            check(fl_decode_sample_ex(model.raw_model(), c, output_ids[0], model.rope_offset(prompt.size(), cache), max_tokens - 1,
                                      eos ? (int64_t)*eos : -1, &s1, output_ids.data() + 1, &n), "Model forward pass failed");
            model.advance(cache, fl_cache_len(c) - len0);
            forwards += fl_cache_len(c) - len0;
        }
        output_ids.resize(ended ? 0 : 1 + n);
        return output_ids;
    }

    // ... a greedy request (temperature < 1e-7, else FL_ERR_UNSUPPORTED) decoded with prompt-lookup drafts: fl_forward for the prompt,
    // ArgMax of its logits, then fl_decode_lookup for the other max_tokens - 1 tokens with the prompt as the search text.  The ids
    // are those of the overloads above (up to bf16 near-ties, include/fastllm_mi355x.h); `forwards` counts the prompt's forward and
    // the verify steps -- the reference's wasted forward behind the last token (C.5) is not run.
    std::vector<uint32_t> generate_ids(const std::vector<uint32_t> &prompt, size_t max_tokens, float temperature,
                                       std::optional<uint32_t> eos, const LookupOptions &lookup, fl_spec_stats *stats = nullptr) {
        require_greedy(temperature);
        cache = M::initialize_cache(device, dtype);
        if (prompt.empty()) throw Error(FL_ERR_BAD_ARGUMENT, "Tokenization error: empty prompt");
        std::vector<uint32_t> output_ids;
        forwards = 0;
        if (stats) *stats = fl_spec_stats{};
        Tensor logits = model.forward(Tensor::from_ids(prompt), 0, cache); forwards++;
        if (max_tokens == 0) return output_ids;
        const uint32_t first = argmax_last(logits.f32(), (size_t)logits.elem_count());
        if (eos && first == *eos) return output_ids;
        output_ids.assign(max_tokens, 0);
        output_ids[0] = first;
        size_t n = 0;
        if (max_tokens > 1) {
            const fl_lookup o = lookup.to_ffi();
            fl_spec_stats st{};
            fl_cache *c = model.raw_cache(cache);
            const size_t len0 = fl_cache_len(c);
            check(fl_decode_lookup(model.raw_model(), c, prompt.data(), prompt.size(), first, model.rope_offset(prompt.size(), cache), max_tokens - 1,
                                   eos ? (int64_t)*eos : -1, &o, output_ids.data() + 1, &n, &st), "Model forward pass failed");
            model.advance(cache, fl_cache_len(c) - len0);
            forwards += (size_t)st.steps;
            if (stats) *stats = st;
        }
        output_ids.resize(1 + n);
        return output_ids;
    }

    // ... and as a stream: one fl_lookup_draft + fl_forward_verify step at a time, every token of a step to `on_token` before the
    // next step (a dropped receiver ends the stream after the step it was in).  Returns the forwards executed.
    template <class OnToken>
    size_t generate_stream_ids(const std::vector<uint32_t> &prompt, size_t max_tokens, float temperature,
                               std::optional<uint32_t> eos, const LookupOptions &lookup, OnToken &&on_token) const {
        require_greedy(temperature);
        M shared = model;
        typename M::Cache own = M::initialize_cache(device, dtype);
        if (prompt.empty()) throw Error(FL_ERR_BAD_ARGUMENT, "Tokenization error: empty prompt");
        size_t n_forwards = 0;
        Tensor logits = shared.forward(Tensor::from_ids(prompt), 0, own); n_forwards++;
        if (max_tokens == 0) return n_forwards;
        uint32_t tok = argmax_last(logits.f32(), (size_t)logits.elem_count());
        if ((eos && tok == *eos) || !on_token(tok)) return n_forwards;
        const fl_lookup o = lookup.to_ffi();
        fl_model_info info; check(fl_model_get_info(shared.raw_model(), &info), "fl_model_get_info");
        fl_cache *c = shared.raw_cache(own);
        std::vector<uint32_t> history(prompt);
        history.push_back(tok);
        size_t emitted = 1, pos = prompt.size();
        uint32_t draft[FL_VERIFY_MAX_DRAFT + 1], got[FL_VERIFY_MAX_DRAFT + 1];
        while (emitted < max_tokens) {
            const size_t rope = shared.rope_offset(pos, own);
            size_t limit = max_tokens - emitted - 1;
            limit = std::min(limit, fl_cache_capacity(c) - fl_cache_len(c) - 1);
            limit = std::min(limit, (size_t)info.cfg.max_position_embeddings - rope - 1);
            if (info.cfg.family != FL_FAMILY_LLAMA && info.cfg.sliding_window > 0) limit = std::min(limit, (size_t)info.cfg.sliding_window);
            size_t nd = 0, n = 0;
            check(fl_lookup_draft(history.data(), history.size(), &o, limit, draft, &nd), "fl_lookup_draft");
            check(fl_forward_verify(shared.raw_model(), c, tok, draft, nd, rope, got, &n, nullptr), "Model forward pass failed");
            n_forwards++;
            shared.advance(own, n);
            pos += n;
            for (size_t i = 0; i < n; i++) {
                if (eos && got[i] == *eos) return n_forwards;
                if (!on_token(got[i])) return n_forwards;
                history.push_back(got[i]);
                if (++emitted == max_tokens) return n_forwards;
            }
            tok = got[n - 1];
        }
        return n_forwards;
    }

    // ... a SAMPLED request decoded with prompt-lookup drafts (fl_decode_lookup_ex): the first token is drawn from the prompt's forward
    // with word 0 (fl_forward_sample_ex), the other max_tokens - 1 by verify steps whose row i is drawn with word 1 + emitted + i and
    // accepted while the draws equal the drafts -- the seeded stream of the SamplingOptions overload above, token k with word k (up to
    // draws that land within the last bits of a boundary, include/fastllm_mi355x.h).  temperature < 1e-7 is the greedy overload's loop.
    std::vector<uint32_t> generate_ids(const std::vector<uint32_t> &prompt, size_t max_tokens, float temperature,
                                       std::optional<uint32_t> eos, const SamplingOptions &opt, const LookupOptions &lookup,
                                       fl_spec_stats *stats = nullptr) {
        cache = M::initialize_cache(device, dtype);
        if (prompt.empty()) throw Error(FL_ERR_BAD_ARGUMENT, "Tokenization error: empty prompt");
        forwards = 0;
        if (stats) *stats = fl_spec_stats{};
        std::vector<uint32_t> output_ids;
        if (max_tokens == 0) { model.forward(Tensor::from_ids(prompt), 0, cache); forwards++; return output_ids; }
        output_ids.assign(max_tokens, 0);
        model.prepare(cache);
        fl_cache *c = model.raw_cache(cache);
        const fl_sampler s0 = opt.to_ffi((double)temperature, 0);
        check(fl_forward_sample_ex(model.raw_model(), c, prompt.data(), prompt.size(), model.rope_offset(0, cache), &s0, &output_ids[0]),
              "Model forward pass failed");
        model.advance(cache, 1); forwards++;
        size_t n = 0;
        const bool ended = eos && output_ids[0] == *eos;
        if (!ended && max_tokens > 1) {
            const fl_sampler s1 = opt.to_ffi((double)temperature, 1);
            const fl_lookup o = lookup.to_ffi();
            fl_spec_stats st{};
            const size_t len0 = fl_cache_len(c);
            check(fl_decode_lookup_ex(model.raw_model(), c, prompt.data(), prompt.size(), output_ids[0], model.rope_offset(prompt.size(), cache),
                                      max_tokens - 1, eos ? (int64_t)*eos : -1, &o, &s1, output_ids.data() + 1, &n, &st), "Model forward pass failed");
            model.advance(cache, fl_cache_len(c) - len0);
            forwards += (size_t)st.steps;
            if (stats) *stats = st;
        }
        output_ids.resize(ended ? 0 : 1 + n);
        return output_ids;
    }

    // ... and as a stream: one fl_lookup_draft + fl_forward_verify_ex step at a time, the draw position (tokens emitted so far) passed
    // along with every call.  Returns the forwards executed.
    template <class OnToken>
    size_t generate_stream_ids(const std::vector<uint32_t> &prompt, size_t max_tokens, float temperature, std::optional<uint32_t> eos,
                               const SamplingOptions &opt, const LookupOptions &lookup, OnToken &&on_token) const {
        M shared = model;
        typename M::Cache own = M::initialize_cache(device, dtype);
        if (prompt.empty()) throw Error(FL_ERR_BAD_ARGUMENT, "Tokenization error: empty prompt");
        size_t n_forwards = 0;
        if (max_tokens == 0) { shared.forward(Tensor::from_ids(prompt), 0, own); return 1; }
        shared.prepare(own);
        fl_cache *c = shared.raw_cache(own);
        uint32_t tok = 0;
        const fl_sampler s0 = opt.to_ffi((double)temperature, 0);
        check(fl_forward_sample_ex(shared.raw_model(), c, prompt.data(), prompt.size(), shared.rope_offset(0, own), &s0, &tok), "Model forward pass failed");
        shared.advance(own, 1); n_forwards++;
        if ((eos && tok == *eos) || !on_token(tok)) return n_forwards;
        const fl_lookup o = lookup.to_ffi();
        fl_model_info info; check(fl_model_get_info(shared.raw_model(), &info), "fl_model_get_info");
        std::vector<uint32_t> history(prompt);
        history.push_back(tok);
        size_t emitted = 1, pos = prompt.size();
        uint32_t draft[FL_VERIFY_MAX_DRAFT + 1], got[FL_VERIFY_MAX_DRAFT + 1];
        while (emitted < max_tokens) {
            const size_t rope = shared.rope_offset(pos, own);
            size_t limit = max_tokens - emitted - 1;
            limit = std::min(limit, fl_cache_capacity(c) - fl_cache_len(c) - 1);
            limit = std::min(limit, (size_t)info.cfg.max_position_embeddings - rope - 1);
            if (info.cfg.family != FL_FAMILY_LLAMA && info.cfg.sliding_window > 0) limit = std::min(limit, (size_t)info.cfg.sliding_window);
            size_t nd = 0, n = 0;
            check(fl_lookup_draft(history.data(), history.size(), &o, limit, draft, &nd), "fl_lookup_draft");
            const fl_sampler sp = opt.to_ffi((double)temperature, emitted);     // token k is drawn with word k
            check(fl_forward_verify_ex(shared.raw_model(), c, tok, draft, nd, rope, &sp, got, &n, nullptr), "Model forward pass failed");
            n_forwards++;
            shared.advance(own, n);
            pos += n;
            for (size_t i = 0; i < n; i++) {
                if (eos && got[i] == *eos) return n_forwards;
                if (!on_token(got[i])) return n_forwards;
                history.push_back(got[i]);
                if (++emitted == max_tokens) return n_forwards;
            }
            tok = got[n - 1];
        }
        return n_forwards;
    }

    // ... a FULL request decoded with prompt-lookup drafts (fl_decode_lookup_lp): penalties and logit_bias (rules), a response format
    // (guide) and log-probs (top_logprobs >= 0 with `out`; < 0: none) no longer take a request out of the lookup loop.  The first token
    // comes from the prompt's forward with the rules and the guide already installed (fl_forward_sample_ex / _lp, word 0), the other
    // max_tokens - 1 from verify steps whose row i sees the rules table and the guide state the plain loop would hold at that step.
    // The ids are those of the rules / guide overloads above with the same options (up to near-ties, include/fastllm_mi355x.h).
    std::vector<uint32_t> generate_ids(const std::vector<uint32_t> &prompt, size_t max_tokens, float temperature,
                                       std::optional<uint32_t> eos, const SamplingOptions &opt, const LookupOptions &lookup,
                                       const LogitRules *rules, const GuideOptions *guide, int top_logprobs = -1, TokenLogprobs *out = nullptr,
                                       fl_spec_stats *stats = nullptr) {
        const bool want_lp = top_logprobs >= 0;
        if (want_lp && !out) throw Error(FL_ERR_BAD_ARGUMENT, "generate_ids: null TokenLogprobs");
        if (top_logprobs > FL_LOGPROBS_MAX_TOP) throw Error(FL_ERR_BAD_ARGUMENT, "generate_ids: top_logprobs out of range");
        cache = M::initialize_cache(device, dtype);
        if (prompt.empty()) throw Error(FL_ERR_BAD_ARGUMENT, "Tokenization error: empty prompt");
        forwards = 0;
        if (stats) *stats = fl_spec_stats{};
        if (out) { *out = TokenLogprobs{}; out->top_n = want_lp ? top_logprobs : 0; }
        std::vector<uint32_t> output_ids;
        if (max_tokens == 0) { model.forward(Tensor::from_ids(prompt), 0, cache); forwards++; return output_ids; }
        const size_t w = want_lp ? (size_t)top_logprobs : 0;
        output_ids.assign(max_tokens, 0);
        if (want_lp) { out->token.assign(max_tokens, 0.f); out->top_ids.assign(max_tokens * w, 0); out->top.assign(max_tokens * w, 0.f); }
        auto lp_at = [&](size_t row) {
            fl_logprobs lp{};
            lp.struct_size = (uint32_t)sizeof(fl_logprobs);
            lp.top_n = (int32_t)w;
            lp.token_logprob = out->token.data() + row;
            lp.top_ids = w ? out->top_ids.data() + row * w : nullptr;
            lp.top_logprobs = w ? out->top.data() + row * w : nullptr;
            return lp;
        };
        model.prepare(cache);
        fl_cache *c = model.raw_cache(cache);
        if (rules) rules->install(model.raw_model(), c, prompt);
        if (guide) guide->install(model.raw_model(), c);
        const fl_sampler s0 = opt.to_ffi((double)temperature, 0);
        if (want_lp) {
            const fl_logprobs lp0 = lp_at(0);
            check(fl_forward_sample_lp(model.raw_model(), c, prompt.data(), prompt.size(), model.rope_offset(0, cache), &s0, &output_ids[0], &lp0),
                  "Model forward pass failed");
        } else {
            check(fl_forward_sample_ex(model.raw_model(), c, prompt.data(), prompt.size(), model.rope_offset(0, cache), &s0, &output_ids[0]),
                  "Model forward pass failed");
        }
        model.advance(cache, 1); forwards++;
        size_t n = 0;
        const bool ended = eos && output_ids[0] == *eos;
        if (!ended && max_tokens > 1) {
            const fl_sampler s1 = opt.to_ffi((double)temperature, 1);
            const fl_lookup o = lookup.to_ffi();
            fl_logprobs lp1{};
            if (want_lp) lp1 = lp_at(1);
            fl_spec_stats st{};
            const size_t len0 = fl_cache_len(c);
            check(fl_decode_lookup_lp(model.raw_model(), c, prompt.data(), prompt.size(), output_ids[0], model.rope_offset(prompt.size(), cache),
                                      max_tokens - 1, eos ? (int64_t)*eos : -1, &o, &s1, want_lp ? &lp1 : nullptr, output_ids.data() + 1, &n, &st),
                  "Model forward pass failed");
            model.advance(cache, fl_cache_len(c) - len0);
            forwards += (size_t)st.steps;
            if (stats) *stats = st;
        }
        const size_t total = ended ? 0 : 1 + n;
        output_ids.resize(total);
        if (want_lp) { out->token.resize(total); out->top_ids.resize(total * w); out->top.resize(total * w); }
        return output_ids;
    }

    // ... and as a stream: one fl_lookup_draft + fl_forward_verify_lp step at a time on the stream's own ruled / guided cache (the call
    // counts its kept rows' inputs and walks the guide itself, so nothing is re-installed between steps), the draw position passed
    // along; on_lp (or nullptr) receives each emitted token's log-probability record ahead of on_token.  Returns the forwards executed.
    template <class OnToken>
    size_t generate_stream_ids(const std::vector<uint32_t> &prompt, size_t max_tokens, float temperature, std::optional<uint32_t> eos,
                               const SamplingOptions &opt, const LookupOptions &lookup, const LogitRules *rules, const GuideOptions *guide,
                               OnToken &&on_token, int top_logprobs = -1,
                               const std::function<void(float, const uint32_t *, const float *)> &on_lp = {}) const {
        const bool want_lp = top_logprobs >= 0;
        if (top_logprobs > FL_LOGPROBS_MAX_TOP) throw Error(FL_ERR_BAD_ARGUMENT, "generate_stream_ids: top_logprobs out of range");
        M shared = model;
        typename M::Cache own = M::initialize_cache(device, dtype);
        if (prompt.empty()) throw Error(FL_ERR_BAD_ARGUMENT, "Tokenization error: empty prompt");
        size_t n_forwards = 0;
        if (max_tokens == 0) { shared.forward(Tensor::from_ids(prompt), 0, own); return 1; }
        shared.prepare(own);
        fl_cache *c = shared.raw_cache(own);
        if (rules) rules->install(shared.raw_model(), c, prompt);
        if (guide) guide->install(shared.raw_model(), c);
        const size_t w = want_lp ? (size_t)top_logprobs : 0;
        float tlp[FL_VERIFY_MAX_DRAFT + 1];
        std::vector<uint32_t> top_ids((FL_VERIFY_MAX_DRAFT + 1) * std::max<size_t>(w, 1));
        std::vector<float> top((FL_VERIFY_MAX_DRAFT + 1) * std::max<size_t>(w, 1));
        fl_logprobs lp{};
        lp.struct_size = (uint32_t)sizeof(fl_logprobs);
        lp.top_n = (int32_t)w;
        lp.token_logprob = tlp;
        lp.top_ids = w ? top_ids.data() : nullptr;
        lp.top_logprobs = w ? top.data() : nullptr;
        auto report = [&](size_t i) { if (want_lp && on_lp) on_lp(tlp[i], top_ids.data() + i * w, top.data() + i * w); };
        uint32_t tok = 0;
        const fl_sampler s0 = opt.to_ffi((double)temperature, 0);
        if (want_lp) check(fl_forward_sample_lp(shared.raw_model(), c, prompt.data(), prompt.size(), shared.rope_offset(0, own), &s0, &tok, &lp), "Model forward pass failed");
        else check(fl_forward_sample_ex(shared.raw_model(), c, prompt.data(), prompt.size(), shared.rope_offset(0, own), &s0, &tok), "Model forward pass failed");
        shared.advance(own, 1); n_forwards++;
        if (eos && tok == *eos) return n_forwards;
        report(0);
        if (!on_token(tok)) return n_forwards;
        const fl_lookup o = lookup.to_ffi();
        fl_model_info info; check(fl_model_get_info(shared.raw_model(), &info), "fl_model_get_info");
        std::vector<uint32_t> history(prompt);
        history.push_back(tok);
        size_t emitted = 1, pos = prompt.size();
        uint32_t draft[FL_VERIFY_MAX_DRAFT + 1], got[FL_VERIFY_MAX_DRAFT + 1];
        while (emitted < max_tokens) {
            const size_t rope = shared.rope_offset(pos, own);
            size_t limit = max_tokens - emitted - 1;
            limit = std::min(limit, fl_cache_capacity(c) - fl_cache_len(c) - 1);
            limit = std::min(limit, (size_t)info.cfg.max_position_embeddings - rope - 1);
            if (info.cfg.family != FL_FAMILY_LLAMA && info.cfg.sliding_window > 0) limit = std::min(limit, (size_t)info.cfg.sliding_window);
            size_t nd = 0, n = 0;
            check(fl_lookup_draft(history.data(), history.size(), &o, limit, draft, &nd), "fl_lookup_draft");
            const fl_sampler sp = opt.to_ffi((double)temperature, emitted);     // token k is drawn with word k
            check(fl_forward_verify_lp(shared.raw_model(), c, tok, draft, nd, rope, &sp, want_lp ? &lp : nullptr, got, &n, nullptr),
                  "Model forward pass failed");
            n_forwards++;
            shared.advance(own, n);
            pos += n;
            for (size_t i = 0; i < n; i++) {
                if (eos && got[i] == *eos) return n_forwards;
                report(i);
                if (!on_token(got[i])) return n_forwards;
                history.push_back(got[i]);
                if (++emitted == max_tokens) return n_forwards;
            }
            tok = got[n - 1];
        }
        return n_forwards;
    }

    // ModelWrapper::generate_stream + generate_tokens_inner (mod.rs:137-238, 268-340) on token ids: the model is CLONED (a
    // reference-count bump, mod.rs:155), the stream gets a FRESH cache of its own (mod.rs:156: this object's `cache` is not
    // touched, so several streams may run on one model at once, each from its own thread -- the reference spawns a task per
    // stream), a seed-0 LogitsProcessor (mod.rs:157-158), and every sampled token goes to `on_token` before the next forward
    // (mod.rs:323-325); `on_token` returning false is the dropped receiver (`tx.send(..).is_err()` -> break).  EOS stops the
    // stream before the token is emitted (mod.rs:312-316).  Returns the number of forwards executed (the one behind the last
    // emitted token included, as in the reference's loop).
    // ... a guided stream (and optionally rules beside the guide): the stream's own cache carries them, every token is selected on the
    // device (fl_forward_sample_ex, one call per token, the draw position passed along) and handed to `on_token` before the next
    // forward.  The ids are those of generate_ids with the same options.  Returns the forwards executed.
    template <class OnToken>
    size_t generate_stream_ids(const std::vector<uint32_t> &prompt, size_t max_tokens, float temperature, std::optional<uint32_t> eos,
                               const SamplingOptions &opt, const GuideOptions &guide, const LogitRules *rules, OnToken &&on_token) const {
        M shared = model;
        typename M::Cache own = M::initialize_cache(device, dtype);
        if (prompt.empty()) throw Error(FL_ERR_BAD_ARGUMENT, "Tokenization error: empty prompt");
        shared.prepare(own);
        fl_cache *c = shared.raw_cache(own);
        if (rules) rules->install(shared.raw_model(), c, prompt);
        guide.install(shared.raw_model(), c);
        size_t pos = 0, n_forwards = 0;
        std::vector<uint32_t> input = prompt, output;
        for (size_t i = 0; i < max_tokens; i++) {
            const fl_sampler sp = opt.to_ffi((double)temperature, i);
            uint32_t next = 0;
            // (rules count decode inputs only: the stream re-installs them with the outputs so far, as a resumed request does)
            if (rules && i > 0) rules->install(shared.raw_model(), c, prompt, output);
            check(fl_forward_sample_ex(shared.raw_model(), c, input.data(), input.size(), shared.rope_offset(pos, own), &sp, &next), "Model forward pass failed");
            shared.advance(own, input.size()); n_forwards++;
            pos += input.size();
            if (eos && next == *eos) break;
            if (!on_token(next)) break;
            output.push_back(next);
            input.assign(1, next);
        }
        return n_forwards;
    }

    template <class OnToken>
    size_t generate_stream_ids(const std::vector<uint32_t> &prompt, size_t max_tokens, float temperature,
                               std::optional<uint32_t> eos, OnToken &&on_token) const {
        return generate_stream_ids(prompt, max_tokens, temperature, eos, SamplingOptions{}, std::forward<OnToken>(on_token));
    }
    template <class OnToken>
    size_t generate_stream_ids(const std::vector<uint32_t> &prompt, size_t max_tokens, float temperature,
                               std::optional<uint32_t> eos, const SamplingOptions &opt, OnToken &&on_token) const {
        M shared = model;                                                  // Arc::new(RwLock::new(model.model.clone()))
        typename M::Cache own = M::initialize_cache(device, dtype);       // one cache per stream
        LogitsProcessor logits_processor(0, (double)temperature, opt.top_p, opt.top_k);
        if (prompt.empty()) throw Error(FL_ERR_BAD_ARGUMENT, "Tokenization error: empty prompt");
        Tensor input = Tensor::from_ids(prompt);                           // mod.rs:283-291
        size_t pos = 0, n_forwards = 0;
        Tensor logits = shared.forward(input, pos, own); n_forwards++;     // mod.rs:296-298
        pos += prompt.size();
        for (size_t i = 0; i < max_tokens; i++) {                          // mod.rs:303
            const uint32_t next = logits_processor.sample(logits.f32(), (size_t)logits.elem_count());   // mod.rs:305-310
            if (eos && next == *eos) break;                                // mod.rs:312-316
            if (!on_token(next)) break;                                    // mod.rs:323-325
            Tensor next_input = Tensor::from_ids({next});                  // mod.rs:328-331
            logits = shared.forward(next_input, pos, own); n_forwards++;   // mod.rs:333-335
            pos += 1;
        }
        return n_forwards;
    }
};

// ------------------------------------------------------------------------------------ K/V reuse across requests
// The reference rebuilds the whole conversation into one prompt per request (api/chat.rs: messages -> format_messages -> generate,
// which takes a fresh cache, mod.rs:370): turn n prefills turns 1 .. n-1 again, and requests that share a system prompt prefill it
// once each.  fl_cache_copy_prefix carries cached positions from one fl_cache to another; the two classes below decide WHICH.
//
// PrefixIndex: pure host code, no GPU.  Up to `entries` id sequences in least-recently-used order (a hit, an insert and an insert
// that found its ids already stored all count as a use).
class PrefixIndex {
  public:
    static constexpr size_t npos = (size_t)-1;
    explicit PrefixIndex(size_t entries) : seqs_(entries), used_(entries, 0) {
        if (entries == 0) throw Error(FL_ERR_BAD_ARGUMENT, "PrefixIndex: at least one entry");
    }
    size_t entries() const { return seqs_.size(); }
    const std::vector<uint32_t> &ids(size_t e) const { return seqs_.at(e); }
    void clear(size_t e) { seqs_.at(e).clear(); used_.at(e) = 0; }

    // (entry, n): n = the longest common prefix of `prompt` with any stored sequence, capped at prompt.size() - 1 (one token at least
    // must be forwarded to obtain logits); ties go to the most recently used entry.  n < max(min_match, 1): a miss, (npos, 0).
    std::pair<size_t, size_t> match(const std::vector<uint32_t> &prompt, size_t min_match) {
        size_t best = npos, best_n = 0;
        for (size_t e = 0; e < seqs_.size(); e++) {
            const size_t n = std::min(common(prompt, seqs_[e]), prompt.empty() ? 0 : prompt.size() - 1);
            if (n > best_n || (n == best_n && n > 0 && used_[e] > used_[best])) { best = e; best_n = n; }
        }
        if (best == npos || best_n < std::max<size_t>(min_match, 1)) return {npos, 0};
        used_[best] = ++clock_;
        return {best, best_n};
    }
    // the entry whose sequence `ids` replaces (its K/V is to be overwritten by the caller), or npos when nothing is stored:
    //   ids is a prefix of a stored sequence (or equal to it): nothing is stored (that entry counts as used);
    //   a stored sequence is a prefix of ids: the longest such entry is extended in place (ties: the most recently used);
    //   otherwise the least recently used entry is taken (never-used entries first, the lowest index among them).
    size_t insert(const std::vector<uint32_t> &ids) {
        if (ids.empty()) return npos;
        size_t covered = npos, ext = npos, lru = 0;
        for (size_t e = 0; e < seqs_.size(); e++) {
            const std::vector<uint32_t> &q = seqs_[e];
            const size_t c = common(ids, q);
            if (c == ids.size() && (covered == npos || used_[e] > used_[covered])) covered = e;
            if (!q.empty() && c == q.size() &&
                (ext == npos || q.size() > seqs_[ext].size() || (q.size() == seqs_[ext].size() && used_[e] > used_[ext]))) ext = e;
            if (used_[e] < used_[lru]) lru = e;
        }
        if (covered != npos) { used_[covered] = ++clock_; return npos; }
        const size_t e = ext != npos ? ext : lru;
        seqs_[e] = ids;
        used_[e] = ++clock_;
        return e;
    }

  private:
    static size_t common(const std::vector<uint32_t> &a, const std::vector<uint32_t> &b) {
        const size_t m = std::min(a.size(), b.size());
        size_t i = 0;
        while (i < m && a[i] == b[i]) i++;
        return i;
    }
    std::vector<std::vector<uint32_t>> seqs_;
    std::vector<uint64_t> used_;                 // 0: never used
    uint64_t clock_ = 0;
};

// PrefixStore: a PrefixIndex plus one fl_cache per entry, all created up front with one capacity -- nothing is allocated on the
// serving path.  An entry's sequence is never longer than what its cache holds.
class PrefixStore {
  public:
    PrefixStore(std::shared_ptr<detail::ModelHandle> model, size_t entries, size_t max_seq, size_t min_match)
        : model_(std::move(model)), index_(entries), cap_(max_seq), min_match_(min_match) {
        if (!model_ || !model_->m) throw Error(FL_ERR_BAD_ARGUMENT, "PrefixStore: no model");
        if (cap_ == 0) throw Error(FL_ERR_BAD_ARGUMENT, "PrefixStore: max_seq must be > 0");
        caches_.resize(entries);
        for (auto &c : caches_) check(fl_cache_create(model_->m, cap_, &c.c), "fl_cache_create");
    }
    size_t capacity() const { return cap_; }
    const PrefixIndex &index() const { return index_; }

    // dst takes the longest stored prefix of `prompt` (fl_cache_copy_prefix); returns its length n -- the caller forwards prompt[n:]
    // at position n -- or 0 on a miss (dst is untouched then)
    size_t lookup_into(fl_cache *dst, const std::vector<uint32_t> &prompt) {
        auto [e, n] = index_.match(prompt, min_match_);
        if (e == PrefixIndex::npos) return 0;
        n = std::min(n, fl_cache_capacity(dst));
        if (n < std::max<size_t>(min_match_, 1)) return 0;
        check(fl_cache_copy_prefix(dst, caches_[e].c, n), "fl_cache_copy_prefix");
        return n;
    }
    // `src` holds the K/V of `ids` (its first ids.size() positions): keep min(ids.size(), fl_cache_len(src), capacity) of them
    void remember(fl_cache *src, const std::vector<uint32_t> &ids) {
        const size_t n = std::min(std::min(ids.size(), fl_cache_len(src)), cap_);
        if (n == 0) return;
        const size_t e = index_.insert(std::vector<uint32_t>(ids.begin(), ids.begin() + (ptrdiff_t)n));
        if (e == PrefixIndex::npos) return;
        try { check(fl_cache_copy_prefix(caches_[e].c, src, n), "fl_cache_copy_prefix"); }
        catch (...) { index_.clear(e); throw; }           // the entry's cache no longer matches any sequence
    }

  private:
    std::shared_ptr<detail::ModelHandle> model_;
    PrefixIndex index_;
    std::vector<detail::CacheHandle> caches_;
    size_t cap_, min_match_;
};

// StreamBatcher option: entries == 0 (default) is the batcher without a store.  min_match: up to 16 tokens a prefill costs one
// short-prompt tile whatever its length (T <= 16 flat), so a shorter match saves nothing.  max_seq: capacity of the
// store's caches, 0 = the slots' capacity.
struct PrefixOptions {
    size_t entries = 0, min_match = 16, max_seq = 0;
};

// StreamBatcher option: on == false (default) admits every request with a forward of its own, exactly as before.  With `on`, the
// requests admitted in one step() whose prompts (with a store: the suffixes behind the reused prefix) have at most max_prompt
// tokens are forwarded together, up to max_tokens tokens (at most 8192, the library's limit) per fl_batch_prefill call: up to about
// 128 rows a forward is one stream of the weights whatever its rows, so n short prompts cost about one.  Longer prompts keep the
// single call.
struct PackedAdmit {
    bool on = false; size_t max_prompt = 256; size_t max_tokens = 2048;
};

// StreamBatcher option: on == false (default) is the batcher exactly as before.  With `on`, every step() drafts for each active
// stream from prompt ++ emitted (fl_lookup_draft; the limit covers the stream's remaining max_tokens, its slot's capacity and the
// model's sliding window), and when no active stream has logit rules or a guide and at least min_drafted ids were drafted in all, the
// step is ONE fl_batch_verify over the active slots -- every stream advances by its accepted drafts + 1 for one read of the weights --
// instead of a chunk of one-token steps.  Per stream the tokens are those of the plain batcher: ArgMax, or the seeded stream with the
// word of each token's index (fl_forward_verify_ex's GUARANTEE).  Where nothing was drafted the step is the existing chunk.
struct BatchLookup {
    bool on = false; LookupOptions lookup; size_t min_drafted = 1;
};

// ------------------------------------------------------------------------------------ concurrent streams, one batched loop
// The reference serves concurrent requests as independent tasks (ModelWrapper::generate_stream spawns one loop per stream,
// mod.rs:137-238), each paying for the whole weight read per token.  StreamBatcher gives the same streams ONE decode loop
// (continuous batching): `slots` caches form an fl_batch; a request waits in a queue until a slot is free, is
// prefilled there alone (fl_forward_sample: its first token), and from then on advances with the others, `chunk` steps per call of
// fl_batch_decode_each -- every stream with its own temperature (a seed-0 sampler of its own, mod.rs:157-158), its own EOS id and
// its own max_tokens.  Per stream the tokens are those of generate_stream_ids with the sampling done on the device (fl_decode_sample):
// sampled, EOS checked before the token is emitted (mod.rs:312-316), the callback's `false` is the dropped receiver (mod.rs:323-325).
// Steps a stream runs past its own end inside a chunk are computed and discarded (its slot's cache is reset on the next admission).
// Not thread-safe: one thread drives submit() / step() (a server would feed it from a channel).
//
// With PrefixOptions.entries > 0 the batcher keeps a PrefixStore: a finished stream leaves the K/V of its prompt and of its reply
// there, and an admitted request whose prompt starts with a stored sequence (turn n of a chat, a shared system prompt) copies that
// prefix into its slot and prefills only the rest, at its token position.  The tokens are those of the batcher without a store.
// Reuse is skipped for a Mistral / Qwen2 prompt longer than the sliding window: within one call the new tokens are masked among
// themselves but a cached prefix is not (fl_forward_verify's note), so prefix + suffix would no longer equal the single call.
// Refused together with counter_positions: with call-counter RoPE offsets a result depends on how many calls produced the cache.
//
// With PackedAdmit.on the admissions of one step() share forwards (fl_batch_prefill); per stream the tokens are those of the single
// admission (the same logits up to fp32 summation order), and every counter but packed_calls / prefill_calls keeps its value.
//
// With BatchLookup.on a step with drafts is one packed verify step (fl_batch_verify) over the active slots; verify_steps / drafted /
// accepted count them.  Refused together with counter_positions, like the prefix store: a verify step's rows sit at token positions.
class StreamBatcher {
  public:
    using OnToken = std::function<bool(uint32_t)>;
    using OnDone = std::function<void(size_t)>;                  // tokens handed to on_token

    // counter_positions: the RoPE offset of a stream's k-th forward is k, not its token position -- what Mistral / Qwen streams
    // see in the reference (quirk C.1: mistral.rs:226,234, qwen.rs:142-143; PosMode::Reference); Llama streams and
    // FASTLLM_POS_MODE=tokens pass token positions
    StreamBatcher(std::shared_ptr<detail::ModelHandle> model, size_t slots, size_t max_seq = 0, size_t chunk = 8, bool counter_positions = false,
                  PrefixOptions prefix = {}, PackedAdmit packed = {}, BatchLookup lookup = {})
        : model_(std::move(model)), chunk_(std::max<size_t>(1, chunk)), counter_(counter_positions), packed_(packed), lookup_(lookup) {
        if (!model_ || !model_->m) throw Error(FL_ERR_BAD_ARGUMENT, "StreamBatcher: no model");
        if (slots < 1 || slots > 64) throw Error(FL_ERR_BAD_ARGUMENT, "StreamBatcher: 1 ... 64 slots");
        if (prefix.entries > 0 && counter_)
            throw Error(FL_ERR_BAD_ARGUMENT, "StreamBatcher: a prefix store needs token positions (with call-counter RoPE offsets a result depends on how "
                                             "many calls produced the cache)");
        if (lookup_.on && counter_)
            throw Error(FL_ERR_BAD_ARGUMENT, "StreamBatcher: batched prompt-lookup needs token positions (the rows of a verify step sit at token positions, "
                                             "not at call-counter RoPE offsets)");
        if (lookup_.on) {
            const fl_lookup o = lookup_.lookup.to_ffi();
            size_t nd = 0;
            check(fl_lookup_draft(nullptr, 0, &o, 0, nullptr, &nd), "BatchLookup");     // the options' own range errors, now and not at the first step
            fl_model_info info; check(fl_model_get_info(model_->m, &info), "fl_model_get_info");
            // the resolved sliding window of a Mistral / Qwen2 model (none, or not positive: no limit), as fl_batch_decode_lookup takes it
            draft_limit_ = info.cfg.family != FL_FAMILY_LLAMA && info.cfg.sliding_window > 0 ? (size_t)info.cfg.sliding_window : (size_t)-1;
            vocab_ = (size_t)info.cfg.vocab_size;
            max_pos_ = (size_t)std::max<int64_t>(0, info.cfg.max_position_embeddings);
        }
        cap_ = max_seq ? max_seq : detail::default_max_seq(model_->m);
        if (cap_ < chunk_ + 1) throw Error(FL_ERR_BAD_ARGUMENT, "StreamBatcher: the caches are shorter than one chunk");
        slots_.resize(slots);
        std::vector<fl_cache *> cs;
        try {
            for (auto &sl : slots_) { check(fl_cache_create(model_->m, cap_, &sl.cache), "fl_cache_create"); cs.push_back(sl.cache); }
            check(fl_batch_create(model_->m, cs.data(), cs.size(), &batch_), "fl_batch_create");
            if (prefix.entries > 0) {
                fl_model_info info; check(fl_model_get_info(model_->m, &info), "fl_model_get_info");
                // the longest prompt a cached prefix may serve: any for Llama, the resolved sliding window for Mistral / Qwen2
                reuse_limit_ = info.cfg.family == FL_FAMILY_LLAMA ? (size_t)-1 : (size_t)std::max<int64_t>(0, info.cfg.sliding_window);
                store_ = std::make_unique<PrefixStore>(model_, prefix.entries, prefix.max_seq ? prefix.max_seq : cap_, prefix.min_match);
            }
        } catch (...) { release(); throw; }
    }
    ~StreamBatcher() { release(); }
    StreamBatcher(const StreamBatcher &) = delete;

    // a request as generate_stream sees it (token ids in, one callback per token out); returns its id
    uint64_t submit(std::vector<uint32_t> prompt, size_t max_tokens, float temperature, std::optional<uint32_t> eos, OnToken on_token,
                    OnDone on_done = {}) {
        return submit(std::move(prompt), max_tokens, temperature, eos, SamplingOptions{}, std::move(on_token), std::move(on_done));
    }
    // ... with the request's own top_p / top_k: one batch mixes ArgMax, Sampling::All and top-p / top-k streams
    uint64_t submit(std::vector<uint32_t> prompt, size_t max_tokens, float temperature, std::optional<uint32_t> eos, const SamplingOptions &opt,
                    OnToken on_token, OnDone on_done = {}) {
        return submit(std::move(prompt), max_tokens, temperature, eos, opt, std::nullopt, std::move(on_token), std::move(on_done));
    }
    // ... and its own logit rules (logit_bias, penalties): installed on the slot's cache for the request's lifetime.  Such a request is
    // admitted with a forward of its own even with PackedAdmit on (fl_batch_prefill's selection does not honour rules), and its rules
    // are removed before the slot's cache is handed back or its K/V goes into the PrefixStore.
    uint64_t submit(std::vector<uint32_t> prompt, size_t max_tokens, float temperature, std::optional<uint32_t> eos, const SamplingOptions &opt,
                    std::optional<LogitRules> rules, OnToken on_token, OnDone on_done = {}) {
        return submit(std::move(prompt), max_tokens, temperature, eos, opt, std::move(rules), std::nullopt, std::move(on_token), std::move(on_done));
    }
    // ... and its own guide: installed on the slot's cache at admission, with the first token selected under it, and removed when the
    // slot is released.  Like a ruled request it is admitted with a forward of its own (fl_batch_prefill's selection honours neither).
    uint64_t submit(std::vector<uint32_t> prompt, size_t max_tokens, float temperature, std::optional<uint32_t> eos, const SamplingOptions &opt,
                    std::optional<LogitRules> rules, std::optional<GuideOptions> guide, OnToken on_token, OnDone on_done = {}) {
        if (guide && !guide->guide) throw Error(FL_ERR_BAD_ARGUMENT, "GuideOptions: no guide");
        if (opt.top_p && *opt.top_p != *opt.top_p) throw Error(FL_ERR_BAD_ARGUMENT, "top_p is NaN");
        if (prompt.empty()) throw Error(FL_ERR_BAD_ARGUMENT, "Tokenization error: empty prompt");
        if (prompt.size() + 1 > cap_) throw Error(FL_ERR_BAD_ARGUMENT, "the prompt does not fit a slot's cache");
        if (!on_token) throw Error(FL_ERR_BAD_ARGUMENT, "null token callback");
        Request r;
        r.id = ++next_id_; r.prompt = std::move(prompt); r.max_tokens = max_tokens; r.temperature = temperature; r.eos = eos; r.opt = opt; r.rules = std::move(rules); r.guide = std::move(guide);
        r.on_token = std::move(on_token); r.on_done = std::move(on_done);
        queue_.push_back(std::move(r));
        return next_id_;
    }

    size_t active() const { size_t n = 0; for (auto &sl : slots_) n += sl.active ? 1 : 0; return n; }
    size_t waiting() const { return queue_.size(); }
    size_t batch_steps = 0;                                        // decode steps the batch has run (all slots advance together)
    size_t prefills = 0;
    size_t prefill_tokens = 0;                                     // prompt tokens the admissions forwarded (with a store: the suffixes only)
    size_t prefix_hits = 0, prefix_tokens_reused = 0;              // admissions that copied a stored prefix, and the positions they copied
    size_t prefill_calls = 0;                                      // forwards the admissions took (without PackedAdmit: == prefills)
    size_t packed_calls = 0;                                       // ... of them fl_batch_prefill calls
    size_t verify_steps = 0, drafted = 0, accepted = 0;            // BatchLookup: packed verify steps, and the ids drafted / accepted in them

    // admit waiting requests into free slots, then one chunk for everybody; false: nothing active and nothing waiting
    bool step() {
        if (packed_.on) admit_packed();
        for (auto &sl : slots_) {
            while (!sl.active && !queue_.empty()) {
                Request r = std::move(queue_.front());             // out of the queue first: a prefill that throws takes its request with it
                queue_.pop_front();
                admit(sl, std::move(r));
            }
        }
        if (active() == 0) return !queue_.empty();
        if (lookup_.on && verify_step()) return true;
        const size_t B = slots_.size();
        size_t n = chunk_, want = 0;
        for (auto &sl : slots_)
            if (sl.active) { n = std::min(n, cap_ - sl.pos); want = std::max(want, sl.req.max_tokens - sl.emitted); }
        n = std::min(n, want);                                     // nobody needs more than `want` further tokens
        std::vector<uint32_t> first(B, 0), out(B * n, 0);
        std::vector<size_t> pos(B, 0), n_out(B, 0);
        std::vector<int64_t> eos(B, -1);
        std::vector<fl_sampler> sp(B, SamplingOptions{}.to_ffi(0.0, 0));
        for (size_t i = 0; i < B; i++) {
            Slot &sl = slots_[i];
            if (!sl.active) { fl_cache_reset(sl.cache); continue; }     // an empty slot computes a throw-away row at position 0
            first[i] = sl.tok; pos[i] = counter_ ? sl.calls : sl.pos;
            if (sl.req.eos) eos[i] = (int64_t)*sl.req.eos;
            sp[i] = sl.req.opt.to_ffi((double)sl.req.temperature, sl.draws);
        }
        check(fl_batch_decode_each_ex(batch_, first.data(), pos.data(), n, eos.data(), sp.data(), out.data(), n_out.data()), "Model forward pass failed");
        batch_steps += n;
        for (size_t i = 0; i < B; i++) {
            Slot &sl = slots_[i];
            if (!sl.active) continue;
            bool done = n_out[i] < n;                              // its EOS came up inside the chunk
            for (size_t k = 0; k < n_out[i]; k++) {
                if (sl.emitted >= sl.req.max_tokens) { done = true; break; }
                sl.emitted++;                                      // (tokens handed to the callback, the refused one included)
                if (store_) sl.held.push_back(out[i * n + k]);
                if (lookup_.on) sl.hist.push_back(out[i * n + k]);
                if (!sl.req.on_token(out[i * n + k])) { done = true; break; }
            }
            if (!done && sl.emitted >= sl.req.max_tokens) done = true;
            sl.pos += n; sl.calls += n; sl.draws += n; sl.tok = out[i * n + n - 1];
            if (!done && sl.pos >= cap_) done = true;               // the slot's cache is full: the stream ends here
            if (done) finish(sl);
        }
        return true;
    }
    void run() { while (step()) {} }

  private:
    struct Request {
        uint64_t id = 0; std::vector<uint32_t> prompt; size_t max_tokens = 0; float temperature = 0.f; std::optional<uint32_t> eos;
        SamplingOptions opt;
        std::optional<LogitRules> rules;
        std::optional<GuideOptions> guide;
        OnToken on_token; OnDone on_done;
    };
    struct Slot {
        fl_cache *cache = nullptr; bool active = false; Request req; size_t pos = 0, calls = 0, emitted = 0; uint32_t tok = 0; uint64_t draws = 0;
        bool ruled = false;                  // the cache has logit rules installed (removed in finish, or by the next admission)
        bool guided = false;                 // ... a guide
        std::vector<uint32_t> held;          // with a store: the prompt and every token handed to the callback
        std::vector<uint32_t> hist;          // with BatchLookup: the same ids, the text the drafts are looked up in
    };

    // BatchLookup: draft for every active slot; false (and nothing done) when the step has to be the plain chunk -- a ruled or guided
    // stream is active, or fewer than min_drafted ids were drafted in all.  Otherwise ONE fl_batch_verify over the active slots and the
    // plain step's bookkeeping per returned id: an EOS, max_tokens or a refused callback finishes the slot and drops the ids behind it.
    bool verify_step() {
        const fl_lookup o = lookup_.lookup.to_ffi();
        std::vector<Slot *> who;
        std::vector<fl_cache *> caches;
        std::vector<uint32_t> ids;
        std::vector<size_t> offsets{0}, pos;
        std::vector<fl_sampler> sp;
        size_t total = 0;
        for (auto &sl : slots_) {
            if (!sl.active) continue;
            if (sl.ruled || sl.guided) return false;
            // room: this step caches the slot's token and its drafts, and hands back at most one id more than it drafted
            size_t limit = std::min(sl.req.max_tokens - sl.emitted, cap_ - sl.pos) - 1;
            limit = std::min(limit, draft_limit_);
            limit = std::min(limit, max_pos_ > sl.pos ? max_pos_ - sl.pos - 1 : 0);     // ... and every row needs a RoPE position
            uint32_t draft[FL_VERIFY_MAX_DRAFT + 1];
            size_t nd = 0;
            check(fl_lookup_draft(sl.hist.data(), sl.hist.size(), &o, limit, draft, &nd), "fl_lookup_draft");
            for (size_t k = 0; k < nd; k++) if (draft[k] >= vocab_) { nd = k; break; }      // (a prompt id the model does not have ends the draft)
            who.push_back(&sl); caches.push_back(sl.cache);
            ids.push_back(sl.tok);
            ids.insert(ids.end(), draft, draft + nd);
            offsets.push_back(ids.size());
            pos.push_back(sl.pos);
            sp.push_back(sl.req.opt.to_ffi((double)sl.req.temperature, sl.draws));
            total += nd;
        }
        if (total < std::max<size_t>(lookup_.min_drafted, 1)) return false;
        std::vector<uint32_t> out(ids.size(), 0);
        std::vector<size_t> n_out(who.size(), 0);
        check(fl_batch_verify(model_->m, caches.data(), caches.size(), ids.data(), offsets.data(), pos.data(), sp.data(), out.data(), n_out.data(), nullptr),
              "Model forward pass failed");
        verify_steps++; drafted += total;
        for (size_t i = 0; i < who.size(); i++) accepted += n_out[i] - 1;
        std::exception_ptr failed;                                 // a callback that throws does not keep the other streams from their ids
        for (size_t i = 0; i < who.size(); i++) {
            Slot &sl = *who[i];
            const uint32_t *got = out.data() + offsets[i];
            const size_t n = n_out[i];
            bool done = false;
            try {
                for (size_t k = 0; k < n; k++) {
                    if (sl.req.eos && got[k] == *sl.req.eos) { done = true; break; }      // EOS is checked before the token is emitted
                    if (sl.emitted >= sl.req.max_tokens) { done = true; break; }
                    sl.emitted++;
                    if (store_) sl.held.push_back(got[k]);
                    sl.hist.push_back(got[k]);
                    if (!sl.req.on_token(got[k])) { done = true; break; }
                }
                if (!done && sl.emitted >= sl.req.max_tokens) done = true;
                sl.pos += n; sl.calls += n; sl.draws += n; sl.tok = got[n - 1];
                if (!done && sl.pos >= cap_) done = true;           // the slot's cache is full: the stream ends here
                if (done) finish(sl);
            } catch (...) {
                if (!failed) failed = std::current_exception();
                if (sl.active) { try { finish(sl); } catch (...) {} }
            }
        }
        if (failed) std::rethrow_exception(failed);
        return true;
    }

    // the slot becomes active only after its prefill succeeded: an exception leaves it free (and the request gone, see step())
    void admit(Slot &sl, Request r) {
        const size_t n = admit_begin(sl, r);
        admit_single(sl, std::move(r), n);
    }
    // the single-prompt forward of an admission; a request's logit rules go onto the slot's cache first (the whole prompt marked as
    // seen, a reused prefix included), so its first token is already selected under them
    void admit_single(Slot &sl, Request r, size_t n) {
        if (r.rules) { r.rules->install(model_->m, sl.cache, r.prompt); sl.ruled = true; }
        if (r.guide) { r.guide->install(model_->m, sl.cache); sl.guided = true; }
        const fl_sampler sp = r.opt.to_ffi((double)r.temperature, 0);
        uint32_t tok = 0;
        check(fl_forward_sample_ex(model_->m, sl.cache, r.prompt.data() + n, r.prompt.size() - n, n, &sp, &tok), "Model forward pass failed");
        prefill_calls++;
        admit_end(sl, std::move(r), n, tok);
    }
    void drop_rules(Slot &sl) {
        if (sl.guided) { sl.guided = false; GuideOptions::remove(model_->m, sl.cache); }
        if (!sl.ruled) return;
        sl.ruled = false;
        LogitRules::remove(model_->m, sl.cache);
    }
    // before the forward: an empty slot cache, or (with a store) the longest stored prefix of the prompt in it; returns its length
    size_t admit_begin(Slot &sl, const Request &r) {
        sl.emitted = 0;
        sl.held.clear();
        drop_rules(sl);                                            // (left behind only by an admission whose forward threw)
        fl_cache_reset(sl.cache);
        size_t n = 0;
        if (store_ && r.prompt.size() <= reuse_limit_) n = store_->lookup_into(sl.cache, r.prompt);
        return n;
    }
    // after it: the counters, the slot's stream state, the first token's EOS / max_tokens / callback cases
    void admit_end(Slot &sl, Request r, size_t n, uint32_t tok) {
        prefills++;
        prefill_tokens += r.prompt.size() - n;
        if (n) { prefix_hits++; prefix_tokens_reused += n; }
        sl.req = std::move(r); sl.active = true;
        if (store_) sl.held = sl.req.prompt;
        if (lookup_.on) { sl.hist = sl.req.prompt; sl.hist.push_back(tok); }
        sl.pos = sl.req.prompt.size(); sl.calls = 1; sl.tok = tok; sl.draws = 1;
        if (sl.req.max_tokens == 0 || (sl.req.eos && tok == *sl.req.eos)) { finish(sl); return; }
        sl.emitted = 1;
        if (store_) sl.held.push_back(tok);
        if (!sl.req.on_token(tok)) { finish(sl); return; }
        if (sl.emitted >= sl.req.max_tokens || sl.pos >= cap_) finish(sl);
    }
    // PackedAdmit: waiting requests are paired with free slots, every slot gets its stored prefix as in admit(), the suffixes of at
    // most max_prompt tokens (and never more than one call holds) go through fl_batch_prefill in groups of at most max_tokens tokens,
    // the longer ones through the single call; then admit()'s bookkeeping per slot.  Repeated while an immediate finish freed a slot
    // and requests still wait.  What throws takes its own requests with it and leaves their slots free, as admit() does: a failed
    // prefix lookup its one request, a failed forward the requests of that call; a request whose bookkeeping throws (its callback, the
    // store) does not keep the other members of its call from theirs.  The requests of the step that were not yet looked at or
    // forwarded go back to the queue's head before the exception leaves.
    void admit_packed() {
        struct Pair { Slot *sl; Request r; size_t n; };
        const size_t max_call = std::min<size_t>(std::max<size_t>(packed_.max_tokens, 1), 8192);
        const size_t max_member = std::min(packed_.max_prompt, max_call);
        for (;;) {
            std::vector<Pair> pairs;
            for (auto &sl : slots_) {
                if (sl.active || queue_.empty()) continue;
                pairs.push_back(Pair{&sl, std::move(queue_.front()), 0});
                queue_.pop_front();
            }
            if (pairs.empty()) return;
            size_t next = 0;                                          // pairs[next ..) still hold their requests
            auto requeue_rest = [&] { for (size_t i = pairs.size(); i > next; i--) queue_.push_front(std::move(pairs[i - 1].r)); };
            for (size_t i = 0; i < pairs.size(); i++) {
                try { pairs[i].n = admit_begin(*pairs[i].sl, pairs[i].r); }
                catch (...) {                                         // this request is gone; nothing has been forwarded yet
                    pairs.erase(pairs.begin() + (std::ptrdiff_t)i);
                    requeue_rest();
                    throw;
                }
            }
            auto suffix = [](const Pair &p) { return p.r.prompt.size() - p.n; };
            auto packable = [&](const Pair &p) { return suffix(p) <= max_member && !p.r.rules && !p.r.guide; };   // (a ruled or guided request takes the single call)
            std::stable_partition(pairs.begin(), pairs.end(), packable);   // the packable pairs first, in slot order
            size_t n_packable = 0;
            while (n_packable < pairs.size() && packable(pairs[n_packable])) n_packable++;
            std::exception_ptr failed;                                // the first bookkeeping failure of a packed call, thrown once its other members are done
            try {
                while (next < n_packable && !failed) {
                    size_t end = next, total = 0;
                    while (end < n_packable && (end == next || total + suffix(pairs[end]) <= max_call)) total += suffix(pairs[end++]);
                    std::vector<fl_cache *> caches;
                    std::vector<uint32_t> ids;
                    std::vector<size_t> offsets{0}, pos;
                    std::vector<fl_sampler> sp;
                    for (size_t i = next; i < end; i++) {
                        const Pair &p = pairs[i];
                        caches.push_back(p.sl->cache);
                        ids.insert(ids.end(), p.r.prompt.begin() + (std::ptrdiff_t)p.n, p.r.prompt.end());
                        offsets.push_back(ids.size());
                        pos.push_back(p.n);
                        sp.push_back(p.r.opt.to_ffi((double)p.r.temperature, 0));
                    }
                    std::vector<uint32_t> toks(end - next, 0);
                    const size_t first = next;
                    next = end;                                       // (forwarded or failed: these requests do not go back)
                    check(fl_batch_prefill(model_->m, caches.data(), caches.size(), ids.data(), offsets.data(), pos.data(), sp.data(), toks.data(), nullptr),
                          "Model forward pass failed");
                    prefill_calls++; packed_calls++;
                    for (size_t i = first; i < end; i++) {
                        try { admit_end(*pairs[i].sl, std::move(pairs[i].r), pairs[i].n, toks[i - first]); }
                        catch (...) { if (!failed) failed = std::current_exception(); }
                    }
                }
                while (next < pairs.size() && !failed) {
                    Pair &p = pairs[next++];
                    admit_single(*p.sl, std::move(p.r), p.n);
                }
            } catch (...) {
                requeue_rest();
                throw;
            }
            if (failed) { requeue_rest(); std::rethrow_exception(failed); }
            bool freed = false;
            for (auto &sl : slots_) freed = freed || !sl.active;
            if (!freed || queue_.empty()) return;
        }
    }
    // With a store the slot's K/V is remembered under the ids it is KNOWN to hold: the prompt and every emitted token except the
    // last (a token's K/V is written by the step that takes it as input), never more than fl_cache_len.
    void finish(Slot &sl) {
        sl.active = false;
        OnDone cb = std::move(sl.req.on_done);
        const size_t n = sl.emitted;
        sl.req = Request{};
        std::exception_ptr failed;
        try { drop_rules(sl); } catch (...) { failed = std::current_exception(); }
        if (store_ && !sl.held.empty()) {
            if (n > 0) sl.held.pop_back();
            try { store_->remember(sl.cache, sl.held); } catch (...) { if (!failed) failed = std::current_exception(); }
            sl.held.clear();
        }
        if (cb) cb(n);
        if (failed) std::rethrow_exception(failed);
    }
    void release() {
        store_.reset();
        if (batch_) { fl_batch_destroy(batch_); batch_ = nullptr; }
        for (auto &sl : slots_) if (sl.cache) { fl_cache_destroy(sl.cache); sl.cache = nullptr; }
    }

    std::shared_ptr<detail::ModelHandle> model_;
    size_t chunk_, cap_ = 0;
    bool counter_ = false;
    PackedAdmit packed_;
    BatchLookup lookup_;
    size_t draft_limit_ = 0, vocab_ = 0, max_pos_ = 0;             // BatchLookup: the model's sliding window (none: no limit), vocabulary and max_position_embeddings
    std::unique_ptr<PrefixStore> store_;                           // null: no prefix reuse
    size_t reuse_limit_ = 0;
    std::vector<Slot> slots_;
    std::deque<Request> queue_;
    fl_batch *batch_ = nullptr;
    uint64_t next_id_ = 0;
};

// ------------------------------------------------------------------------------------ embeddings.rs
// trait EmbeddingModel (embeddings.rs:17-38) and its one implementation MiniLMModel (:245-456) on token ids: the tokenizer and
// do_lower_case stay on the host side of the caller, as for the decoder.  The forward runs on the GPU (fl_encoder_*); Device::Cpu --
// where the reference runs it (:289) -- is rejected.
struct BertConfig {                           // embeddings.rs:46-54 (+ vocab_size: the reference takes it from the tokenizer, :301-303)
    size_t hidden_size = 0, num_attention_heads = 0, num_hidden_layers = 0, intermediate_size = 0, max_position_embeddings = 0;
    double layer_norm_eps = 0;
    std::optional<size_t> vocab_size;         // absent: the rows of embeddings.word_embeddings.weight
    static BertConfig from_json(const std::string &text) {
        detail::JsonFlat j(text);
        BertConfig c;
        c.hidden_size = j.usize("hidden_size");
        c.num_attention_heads = j.usize("num_attention_heads");
        c.num_hidden_layers = j.usize("num_hidden_layers");
        c.intermediate_size = j.usize("intermediate_size");
        c.max_position_embeddings = j.usize("max_position_embeddings");
        c.layer_norm_eps = j.num("layer_norm_eps");
        c.vocab_size = j.opt_usize("vocab_size");
        return c;
    }
};

struct EmbeddingOutput {                      // embeddings.rs:10-15
    std::vector<float> embeddings;
    std::string model;
    size_t token_count = 0;
};

struct EmbeddingOptions {                     // no counterpart in the reference, whose forward is fixed: tanh GELU, no token-type row
    fl_activation activation = FL_ACT_GELU_TANH;
    bool add_token_type0 = false;             // HF's BertModel adds embeddings.token_type_embeddings.weight[0]
    size_t max_batch_tokens = 0;              // 0: the library's default
};

class EmbeddingModel {
  public:
    EmbeddingModel(const BertConfig &cfg, const TensorMap &tensors, DType dtype, const Device &device, std::string model_id = "",
                   const EmbeddingOptions &opt = EmbeddingOptions())
        : model_id_(std::move(model_id)), hidden_(cfg.hidden_size) {
        if (device.is_cpu())
            throw Error(FL_ERR_NO_DEVICE, "the MI355X backend has no CPU path: pass Device::mi355x(..) (the reference's MiniLM runs on Device::Cpu, embeddings.rs:289)");
        if (device.ordinals.size() != 1) throw Error(FL_ERR_UNSUPPORTED, "the encoder runs on one GPU");
        std::vector<fl_tensor> arr;
        arr.reserve(tensors.size());
        size_t vocab = cfg.vocab_size.value_or(0);
        for (auto &kv : tensors) {
            fl_tensor t{};
            t.name = kv.first.c_str(); t.dtype = (int32_t)kv.second.dtype; t.ndim = (int32_t)kv.second.shape.size();
            if (t.ndim > 4) throw Error(FL_ERR_SHAPE_MISMATCH, "tensor " + kv.first + " has rank > 4");
            for (int i = 0; i < t.ndim; i++) t.shape[i] = kv.second.shape[i];
            t.data = kv.second.data; t.device = kv.second.device;
            arr.push_back(t);
            if (!cfg.vocab_size && kv.first == "embeddings.word_embeddings.weight" && t.ndim == 2) vocab = (size_t)t.shape[0];
        }
        fl_encoder_config c{};
        c.struct_size = (uint32_t)sizeof c; c.activation = opt.activation; c.add_token_type0 = opt.add_token_type0 ? 1 : 0;
        c.hidden_size = (int64_t)cfg.hidden_size; c.intermediate_size = (int64_t)cfg.intermediate_size;
        c.num_hidden_layers = (int64_t)cfg.num_hidden_layers; c.num_attention_heads = (int64_t)cfg.num_attention_heads;
        c.max_position_embeddings = (int64_t)cfg.max_position_embeddings; c.vocab_size = (int64_t)vocab;
        c.max_batch_tokens = (int64_t)opt.max_batch_tokens; c.layer_norm_eps = cfg.layer_norm_eps;
        check(fl_encoder_create(&c, arr.data(), arr.size(), (int32_t)dtype, device.ordinals[0], &enc_), "Failed to initialize embedding model");
    }
    ~EmbeddingModel() { if (enc_) fl_encoder_release(enc_); }
    EmbeddingModel(const EmbeddingModel &) = delete;
    EmbeddingModel &operator=(const EmbeddingModel &) = delete;

    // EmbeddingModel::embed (embeddings.rs:396-447) behind the tokenizer: forward, mean pooling, L2 normalisation
    EmbeddingOutput embed_ids(const std::vector<uint32_t> &ids) const {
        const size_t offsets[2] = {0, ids.size()};
        EmbeddingOutput out;
        out.embeddings.resize(hidden_);
        check(fl_encoder_embed(enc_, ids.data(), offsets, 1, out.embeddings.data()), "Failed to embed");
        out.model = model_id_; out.token_count = ids.size();
        return out;
    }
    // many texts in one packed call (new capability: the reference embeds one text at a time); result i is embed_ids(seqs[i])
    std::vector<EmbeddingOutput> embed_batch_ids(const std::vector<std::vector<uint32_t>> &seqs) const {
        std::vector<uint32_t> ids;
        std::vector<size_t> offsets{0};
        for (auto &s : seqs) { ids.insert(ids.end(), s.begin(), s.end()); offsets.push_back(ids.size()); }
        std::vector<float> flat(seqs.size() * hidden_);
        check(fl_encoder_embed(enc_, ids.data(), offsets.data(), seqs.size(), flat.data()), "Failed to embed");
        std::vector<EmbeddingOutput> out(seqs.size());
        for (size_t i = 0; i < seqs.size(); i++) {
            out[i].embeddings.assign(flat.begin() + i * hidden_, flat.begin() + (i + 1) * hidden_);
            out[i].model = model_id_; out[i].token_count = seqs[i].size();
        }
        return out;
    }
    std::string model_id() const { return model_id_; }
    size_t embedding_size() const { return hidden_; }           // the model's hidden_size (the reference hard-codes 384, :453-455)
    // compute_similarity (embeddings.rs:22-37): the cosine, in f32 and in the reference's order of operations
    float compute_similarity_ids(const std::vector<uint32_t> &a, const std::vector<uint32_t> &b) const {
        const std::vector<float> v1 = embed_ids(a).embeddings, v2 = embed_ids(b).embeddings;
        float dot = 0.f, n1 = 0.f, n2 = 0.f;
        for (size_t i = 0; i < v1.size(); i++) dot += v1[i] * v2[i];
        for (float x : v1) n1 += x * x;
        for (float x : v2) n2 += x * x;
        return dot / (std::sqrt(n1) * std::sqrt(n2));
    }
    static const char *get_family() { return "bert"; }          // embeddings.rs:458-466
    static bool supports_architecture(const std::string &a) { return a == "BertModel" || a == "RobertaModel" || a == "DebertaModel"; }

  private:
    fl_encoder *enc_ = nullptr;
    std::string model_id_;
    size_t hidden_;
};

// ------------------------------------------------------------------------------------ decoder-model embeddings
// The same surface over an fl_model (fl_batch_embed): the embedding checkpoints that are decoder models -- e5-mistral / SFR /
// Linq-Embed-Mistral (LAST + CAUSAL), gte-Qwen2 (LAST + FULL), LLM2Vec Llama (MEAN + FULL).  No counterpart in the reference, whose
// /v1/embeddings serves MiniLM only.  Tokenising (and appending EOS where the checkpoint wants it) is the caller's.  The object owns
// its caches: one caller at a time.
struct DecoderEmbeddingOptions {
    fl_pooling pooling = FL_POOL_LAST;        // LAST / MEAN / FIRST (one vector per text; FL_POOL_NONE is the C ABI's)
    fl_attn_mask mask = FL_MASK_CAUSAL;
    bool normalize = true;
    size_t dimensions = 0;                    // 0: hidden_size
    size_t slots = 64;                        // caches in the pool = texts per fl_batch_embed call, 1..64
    size_t max_seq = 0;                       // capacity of each; 0: detail::default_max_seq
};

class DecoderEmbeddingModel {
  public:
    static constexpr size_t kMaxMembers = 64, kMaxTokens = 8192;      // fl_batch_embed's limits per call
    DecoderEmbeddingModel(std::shared_ptr<detail::ModelHandle> model, const DecoderEmbeddingOptions &opt = DecoderEmbeddingOptions(),
                          std::string model_id = "")
        : model_(std::move(model)), opt_(opt), model_id_(std::move(model_id)) {
        if (!model_ || !model_->m) throw Error(FL_ERR_BAD_ARGUMENT, "null model");
        fl_model_info info; check(fl_model_get_info(model_->m, &info), "fl_model_get_info");
        hidden_ = (size_t)info.cfg.hidden_size;
        if (opt_.pooling == FL_POOL_NONE) throw Error(FL_ERR_BAD_ARGUMENT, "DecoderEmbeddingModel returns one vector per text: FL_POOL_NONE is fl_batch_embed's");
        if (opt_.slots < 1 || opt_.slots > kMaxMembers) throw Error(FL_ERR_BAD_ARGUMENT, "DecoderEmbeddingModel: 1..64 slots");
        if (opt_.dimensions > hidden_) throw Error(FL_ERR_BAD_ARGUMENT, "DecoderEmbeddingModel: dimensions exceeds the hidden size");
        const size_t cap = opt_.max_seq ? opt_.max_seq : detail::default_max_seq(model_->m);
        caches_.resize(opt_.slots);
        for (auto &c : caches_) check(fl_cache_create(model_->m, cap, &c.c), "Failed to create an embedding cache");
    }
    DecoderEmbeddingModel(const DecoderEmbeddingModel &) = delete;
    DecoderEmbeddingModel &operator=(const DecoderEmbeddingModel &) = delete;

    EmbeddingOutput embed_ids(const std::vector<uint32_t> &ids) { return embed_batch_ids({ids})[0]; }
    // Any number of texts: cut into calls of at most `slots` members and 8192 tokens, in order; the pool's caches are reset per call.
    // Result i agrees with embed_ids(seqs[i]): bit-identical where both calls fall into one of the planner's row-count regimes, else as
    // two runs that sum in different orders agree (the row-wise projections are chosen by a call's total rows, as in fl_batch_prefill).
    std::vector<EmbeddingOutput> embed_batch_ids(const std::vector<std::vector<uint32_t>> &seqs) {
        const size_t dims = embedding_size();
        std::vector<EmbeddingOutput> out(seqs.size());
        fl_embed e{};
        e.struct_size = (uint32_t)sizeof e; e.pooling = opt_.pooling; e.mask = opt_.mask; e.normalize = opt_.normalize ? 1 : 0;
        e.dimensions = (int64_t)opt_.dimensions;
        size_t i = 0;
        while (i < seqs.size()) {
            std::vector<uint32_t> ids;
            std::vector<size_t> offsets{0};
            size_t j = i;
            // (a text beyond 8192 tokens goes alone and the library says why it cannot be embedded)
            while (j < seqs.size() && j - i < caches_.size() && (j == i || ids.size() + seqs[j].size() <= kMaxTokens)) {
                ids.insert(ids.end(), seqs[j].begin(), seqs[j].end());
                offsets.push_back(ids.size());
                j++;
            }
            const size_t n = j - i;
            std::vector<fl_cache *> cs(n);
            for (size_t k = 0; k < n; k++) { cs[k] = caches_[k].c; fl_cache_reset(cs[k]); }
            const std::vector<size_t> pos(n, 0);
            std::vector<float> flat(n * dims);
            check(fl_batch_embed(model_->m, cs.data(), n, ids.data(), offsets.data(), pos.data(), &e, flat.data()), "Failed to embed");
            // (under FL_MASK_FULL the caches now hold the full-mask model's K/V: they are reset before their next use, above)
            for (size_t k = 0; k < n; k++) {
                out[i + k].embeddings.assign(flat.begin() + k * dims, flat.begin() + (k + 1) * dims);
                out[i + k].model = model_id_; out[i + k].token_count = seqs[i + k].size();
            }
            calls_++;
            i = j;
        }
        return out;
    }
    std::string model_id() const { return model_id_; }
    size_t embedding_size() const { return opt_.dimensions ? opt_.dimensions : hidden_; }
    size_t calls() const { return calls_; }                       // fl_batch_embed calls so far
    // the cosine, as EmbeddingModel::compute_similarity_ids forms it
    float compute_similarity_ids(const std::vector<uint32_t> &a, const std::vector<uint32_t> &b) {
        const std::vector<float> v1 = embed_ids(a).embeddings, v2 = embed_ids(b).embeddings;
        float dot = 0.f, n1 = 0.f, n2 = 0.f;
        for (size_t i = 0; i < v1.size(); i++) dot += v1[i] * v2[i];
        for (float x : v1) n1 += x * x;
        for (float x : v2) n2 += x * x;
        return dot / (std::sqrt(n1) * std::sqrt(n2));
    }

  private:
    std::shared_ptr<detail::ModelHandle> model_;
    DecoderEmbeddingOptions opt_;
    std::string model_id_;
    size_t hidden_ = 0, calls_ = 0;
    std::vector<detail::CacheHandle> caches_;
};

}  // namespace fastllm
