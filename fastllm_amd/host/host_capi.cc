// host_capi.cc -- a small C surface over fastllm_host.hpp so that pytest (ctypes) can drive the C++
// mirror of the reference's trait layer.  Built into fastllm_amd/lib/libfastllm_host.so.
#include <cstdio>
#include <string>

#include "fastllm_host.hpp"
#include "safetensors.hpp"

using namespace fastllm;

namespace {
thread_local std::string g_err;

struct Handle {
    int family;                               // 0 llama, 1 mistral, 2 qwen
    std::unique_ptr<Model<LlamaWithConfig>> llama;
    std::unique_ptr<Model<MistralWithConfig>> mistral;
    std::unique_ptr<Model<QwenWithConfig>> qwen;
};

template <class F> int guard(F &&f) {
    try { return f(); }
    catch (const Error &e) { g_err = e.what(); return e.code ? e.code : -100; }
    catch (const Panic &e) { g_err = std::string("panic: ") + e.what(); return -101; }
    catch (const std::exception &e) { g_err = e.what(); return -102; }
}

TensorMap to_map(const fl_tensor *ts, size_t n) {
    TensorMap m;
    for (size_t i = 0; i < n; i++) {
        Tensor t; t.dtype = (DType)ts[i].dtype; t.data = ts[i].data; t.device = ts[i].device;
        for (int d = 0; d < ts[i].ndim; d++) t.shape.push_back(ts[i].shape[d]);
        m[ts[i].name] = t;
    }
    return m;
}
}  // namespace

extern "C" {

const char *flh_last_error(void) { return g_err.c_str(); }

const char *flh_get_family(int family) {
    switch (family) { case 0: return LlamaWithConfig::get_family(); case 1: return MistralWithConfig::get_family(); case 2: return QwenWithConfig::get_family(); }
    return "";
}

int flh_supports_architecture(int family, const char *arch) {
    switch (family) {
        case 0: return LlamaWithConfig::supports_architecture(arch);
        case 1: return MistralWithConfig::supports_architecture(arch);
        case 2: return QwenWithConfig::supports_architecture(arch);
    }
    return 0;
}

// parse config.json and run the family's validation; out (optional) receives the resolved fl_config
int flh_config_check(int family, const char *json, fl_config *out) {
    return guard([&] {
        BaseModelConfig c = BaseModelConfig::from_json(json);
        if (family == 1) MistralWithConfig::validate(c);
        if (family == 2) {
            try { c.validate_head_dimensions(); c.validate_gqa_config(); }
            catch (const Error &e) { throw Panic(e.what()); }
        }
        if (out) *out = c.to_fl((fl_family)family, family == 2);
        return 0;
    });
}

int flh_model_create(int family, const char *config_json, const fl_tensor *tensors, size_t n, int dtype,
                     int device_ordinal, void **out) {
    return guard([&] {
        BaseModelConfig cfg = BaseModelConfig::from_json(config_json);
        TensorMap map = to_map(tensors, n);
        Device dev = device_ordinal < 0 ? Device::cpu() : Device::mi355x(device_ordinal);
        auto h = std::make_unique<Handle>();
        h->family = family;
        if (family == 0) { auto r = LlamaWithConfig::initialize_model(cfg, map, (DType)dtype, dev); h->llama = std::make_unique<Model<LlamaWithConfig>>(r.first, dev, r.second); }
        else if (family == 1) { auto r = MistralWithConfig::initialize_model(cfg, map, (DType)dtype, dev); h->mistral = std::make_unique<Model<MistralWithConfig>>(r.first, dev, r.second); }
        else if (family == 2) { auto r = QwenWithConfig::initialize_model(cfg, map, (DType)dtype, dev); h->qwen = std::make_unique<Model<QwenWithConfig>>(r.first, dev, r.second); }
        else throw Error(FL_ERR_BAD_ARGUMENT, "unknown family");
        *out = h.release();
        return 0;
    });
}

// load_model::<M>(dir) (huggingface.rs:18-139 minus Hub download and tokenizer): the family is chosen from
// config.json's architectures[0] the way the registry does (model_registry.rs:169-182)
int flh_load_dir(const char *dir, int dtype, int device_ordinal, void **out, int *family_out) {
    return guard([&] {
        const std::string d(dir);
        const std::string arch = architecture_of(read_text(d + "/config.json"));
        const char *fam = get_family_from_architecture(arch);
        if (!fam) throw Error(FL_ERR_BAD_CONFIG, "Unsupported architecture " + arch);
        Device dev = device_ordinal < 0 ? Device::cpu() : Device::mi355x(device_ordinal);
        auto h = std::make_unique<Handle>();
        const std::string f(fam);
        if (f == "Llama") { h->family = 0; h->llama = std::make_unique<Model<LlamaWithConfig>>(load_model<LlamaWithConfig>(d, (DType)dtype, dev)); }
        else if (f == "Mistral") { h->family = 1; h->mistral = std::make_unique<Model<MistralWithConfig>>(load_model<MistralWithConfig>(d, (DType)dtype, dev)); }
        else { h->family = 2; h->qwen = std::make_unique<Model<QwenWithConfig>>(load_model<QwenWithConfig>(d, (DType)dtype, dev)); }
        if (family_out) *family_out = h->family;
        *out = h.release();
        return 0;
    });
}

// parse a checkpoint directory on the host only: number of tensors, and for `name` its dtype / shape /
// a byte checksum (sum of bytes mod 2^64) so tests can compare with an independent reader
int flh_checkpoint_probe(const char *dir, const char *name, size_t *n_tensors, int *dtype, int *ndim, int64_t shape[4],
                         uint64_t *byte_sum) {
    return guard([&] {
        Checkpoint ck(dir);
        if (n_tensors) *n_tensors = ck.tensors.size();
        if (name) {
            auto it = ck.tensors.find(name);
            if (it == ck.tensors.end()) throw Error(FL_ERR_MISSING_TENSOR, std::string("cannot find tensor ") + name);
            const Tensor &t = it->second;
            *dtype = (int)t.dtype; *ndim = (int)t.shape.size();
            size_t cnt = 1;
            for (size_t i = 0; i < t.shape.size() && i < 4; i++) { shape[i] = t.shape[i]; cnt *= (size_t)t.shape[i]; }
            const size_t bytes = cnt * (t.dtype == DType::F32 ? 4 : 2);
            uint64_t sum = 0;
            const unsigned char *p = static_cast<const unsigned char *>(t.data);
            for (size_t i = 0; i < bytes; i++) sum += p[i];
            *byte_sum = sum;
        }
        return 0;
    });
}

void flh_model_destroy(void *h) { delete static_cast<Handle *>(h); }

// Model<M>::generate on token ids (mod.rs:363-463)
int flh_generate(void *hv, const uint32_t *prompt, size_t T, size_t max_tokens, float temperature, int64_t eos,
                 uint32_t *out_tokens, size_t *n_out, size_t *forwards) {
    return guard([&] {
        Handle *h = static_cast<Handle *>(hv);
        std::vector<uint32_t> p(prompt, prompt + T), r;
        std::optional<uint32_t> e = eos >= 0 ? std::optional<uint32_t>((uint32_t)eos) : std::nullopt;
        size_t fw = 0;
        if (h->llama) { r = h->llama->generate_ids(p, max_tokens, temperature, e); fw = h->llama->forwards; }
        else if (h->mistral) { r = h->mistral->generate_ids(p, max_tokens, temperature, e); fw = h->mistral->forwards; }
        else { r = h->qwen->generate_ids(p, max_tokens, temperature, e); fw = h->qwen->forwards; }
        for (size_t i = 0; i < r.size(); i++) out_tokens[i] = r[i];
        *n_out = r.size();
        if (forwards) *forwards = fw;
        return 0;
    });
}

// ... with log-probabilities (generate_ids with top_logprobs): token_logprob [max_tokens], top_ids / top_logprobs [max_tokens][top_n]
// (may be null when top_n == 0); top_p <= 0 and top_k <= 0: off
int flh_generate_logprobs(void *hv, const uint32_t *prompt, size_t T, size_t max_tokens, float temperature, int64_t eos, double top_p,
                          int64_t top_k, int top_n, uint32_t *out_tokens, size_t *n_out, float *token_logprob, uint32_t *top_ids,
                          float *top_logprobs, size_t *forwards) {
    return guard([&] {
        Handle *h = static_cast<Handle *>(hv);
        std::vector<uint32_t> p(prompt, prompt + T), r;
        std::optional<uint32_t> e = eos >= 0 ? std::optional<uint32_t>((uint32_t)eos) : std::nullopt;
        SamplingOptions opt;
        if (top_p > 0) opt.top_p = top_p;
        if (top_k > 0) opt.top_k = (size_t)top_k;
        TokenLogprobs lp;
        size_t fw = 0;
        if (h->llama) { r = h->llama->generate_ids(p, max_tokens, temperature, e, opt, top_n, &lp); fw = h->llama->forwards; }
        else if (h->mistral) { r = h->mistral->generate_ids(p, max_tokens, temperature, e, opt, top_n, &lp); fw = h->mistral->forwards; }
        else { r = h->qwen->generate_ids(p, max_tokens, temperature, e, opt, top_n, &lp); fw = h->qwen->forwards; }
        for (size_t i = 0; i < r.size(); i++) { out_tokens[i] = r[i]; token_logprob[i] = lp.token[i]; }
        for (size_t i = 0; i < lp.top_ids.size(); i++) { top_ids[i] = lp.top_ids[i]; top_logprobs[i] = lp.top[i]; }
        *n_out = r.size();
        if (forwards) *forwards = fw;
        return 0;
    });
}

// Model<M>::score_ids: target_logprob / target_rank [T], top_ids / top_logprobs [T][top_n] (may be null when top_n == 0)
int flh_score_ids(void *hv, const uint32_t *ids, size_t T, int top_n, float *target_logprob, uint32_t *target_rank, uint32_t *top_ids,
                  float *top_logprobs) {
    return guard([&] {
        Handle *h = static_cast<Handle *>(hv);
        std::vector<uint32_t> p(ids, ids + T);
        const ScoredTokens r = h->llama ? h->llama->score_ids(p, top_n) : h->mistral ? h->mistral->score_ids(p, top_n) : h->qwen->score_ids(p, top_n);
        for (size_t i = 0; i < r.token.size(); i++) { target_logprob[i] = r.token[i]; target_rank[i] = r.rank[i]; }
        for (size_t i = 0; i < r.top_ids.size(); i++) { top_ids[i] = r.top_ids[i]; top_logprobs[i] = r.top[i]; }
        return 0;
    });
}

namespace {
LogitRules make_rules(size_t n_bias, const uint32_t *bias_ids, const float *bias_values, float rp, float fp, float pp) {
    LogitRules r;
    for (size_t i = 0; i < n_bias; i++) r.logit_bias.emplace_back(bias_ids[i], bias_values[i]);
    r.repetition_penalty = rp; r.frequency_penalty = fp; r.presence_penalty = pp;
    return r;
}
}  // namespace

// ... with logit rules (generate_ids with LogitRules): n_bias (id, value) pairs and the three penalties; top_p <= 0 and top_k <= 0: off
int flh_generate_rules(void *hv, const uint32_t *prompt, size_t T, size_t max_tokens, float temperature, int64_t eos, double top_p,
                       int64_t top_k, size_t n_bias, const uint32_t *bias_ids, const float *bias_values, float repetition_penalty,
                       float frequency_penalty, float presence_penalty, uint32_t *out_tokens, size_t *n_out, size_t *forwards) {
    return guard([&] {
        Handle *h = static_cast<Handle *>(hv);
        std::vector<uint32_t> p(prompt, prompt + T), r;
        std::optional<uint32_t> e = eos >= 0 ? std::optional<uint32_t>((uint32_t)eos) : std::nullopt;
        SamplingOptions opt;
        if (top_p > 0) opt.top_p = top_p;
        if (top_k > 0) opt.top_k = (size_t)top_k;
        const LogitRules rules = make_rules(n_bias, bias_ids, bias_values, repetition_penalty, frequency_penalty, presence_penalty);
        size_t fw = 0;
        if (h->llama) { r = h->llama->generate_ids(p, max_tokens, temperature, e, opt, rules); fw = h->llama->forwards; }
        else if (h->mistral) { r = h->mistral->generate_ids(p, max_tokens, temperature, e, opt, rules); fw = h->mistral->forwards; }
        else { r = h->qwen->generate_ids(p, max_tokens, temperature, e, opt, rules); fw = h->qwen->forwards; }
        for (size_t i = 0; i < r.size(); i++) out_tokens[i] = r[i];
        *n_out = r.size();
        if (forwards) *forwards = fw;
        return 0;
    });
}

// ... a greedy request with prompt-lookup drafts (LookupOptions); stream != 0: through generate_stream_ids' lookup overload.
// stats (optional): steps, drafted, accepted of the non-stream form
int flh_generate_lookup(void *hv, const uint32_t *prompt, size_t T, size_t max_tokens, float temperature, int64_t eos, int max_draft,
                        int ngram_max, int ngram_min, int stream, uint32_t *out_tokens, size_t *n_out, size_t *forwards, uint64_t stats[3]) {
    return guard([&] {
        Handle *h = static_cast<Handle *>(hv);
        std::vector<uint32_t> p(prompt, prompt + T), r;
        std::optional<uint32_t> e = eos >= 0 ? std::optional<uint32_t>((uint32_t)eos) : std::nullopt;
        LookupOptions lk; lk.max_draft = max_draft; lk.ngram_max = ngram_max; lk.ngram_min = ngram_min;
        fl_spec_stats st{};
        size_t fw = 0;
        auto cb = [&](uint32_t t) { r.push_back(t); return true; };
        if (stream) {
            if (h->llama) fw = h->llama->generate_stream_ids(p, max_tokens, temperature, e, lk, cb);
            else if (h->mistral) fw = h->mistral->generate_stream_ids(p, max_tokens, temperature, e, lk, cb);
            else fw = h->qwen->generate_stream_ids(p, max_tokens, temperature, e, lk, cb);
        } else if (h->llama) { r = h->llama->generate_ids(p, max_tokens, temperature, e, lk, &st); fw = h->llama->forwards; }
        else if (h->mistral) { r = h->mistral->generate_ids(p, max_tokens, temperature, e, lk, &st); fw = h->mistral->forwards; }
        else { r = h->qwen->generate_ids(p, max_tokens, temperature, e, lk, &st); fw = h->qwen->forwards; }
        for (size_t i = 0; i < r.size(); i++) out_tokens[i] = r[i];
        *n_out = r.size();
        if (forwards) *forwards = fw;
        if (stats) { stats[0] = st.steps; stats[1] = st.drafted; stats[2] = st.accepted; }
        return 0;
    });
}

// ... a SAMPLED request with prompt-lookup drafts (SamplingOptions + LookupOptions); top_p <= 0 and top_k <= 0: off; stream != 0: through
// generate_stream_ids' overload.  stats (optional): steps, drafted, accepted of the non-stream form
int flh_generate_lookup_sample(void *hv, const uint32_t *prompt, size_t T, size_t max_tokens, float temperature, int64_t eos, double top_p,
                               int64_t top_k, int max_draft, int ngram_max, int ngram_min, int stream, uint32_t *out_tokens, size_t *n_out,
                               size_t *forwards, uint64_t stats[3]) {
    return guard([&] {
        Handle *h = static_cast<Handle *>(hv);
        std::vector<uint32_t> p(prompt, prompt + T), r;
        std::optional<uint32_t> e = eos >= 0 ? std::optional<uint32_t>((uint32_t)eos) : std::nullopt;
        SamplingOptions opt;
        if (top_p > 0) opt.top_p = top_p;
        if (top_k > 0) opt.top_k = (size_t)top_k;
        LookupOptions lk; lk.max_draft = max_draft; lk.ngram_max = ngram_max; lk.ngram_min = ngram_min;
        fl_spec_stats st{};
        size_t fw = 0;
        auto cb = [&](uint32_t t) { r.push_back(t); return true; };
        if (stream) {
            if (h->llama) fw = h->llama->generate_stream_ids(p, max_tokens, temperature, e, opt, lk, cb);
            else if (h->mistral) fw = h->mistral->generate_stream_ids(p, max_tokens, temperature, e, opt, lk, cb);
            else fw = h->qwen->generate_stream_ids(p, max_tokens, temperature, e, opt, lk, cb);
        } else if (h->llama) { r = h->llama->generate_ids(p, max_tokens, temperature, e, opt, lk, &st); fw = h->llama->forwards; }
        else if (h->mistral) { r = h->mistral->generate_ids(p, max_tokens, temperature, e, opt, lk, &st); fw = h->mistral->forwards; }
        else { r = h->qwen->generate_ids(p, max_tokens, temperature, e, opt, lk, &st); fw = h->qwen->forwards; }
        for (size_t i = 0; i < r.size(); i++) out_tokens[i] = r[i];
        *n_out = r.size();
        if (forwards) *forwards = fw;
        if (stats) { stats[0] = st.steps; stats[1] = st.drafted; stats[2] = st.accepted; }
        return 0;
    });
}

// ModelWrapper::generate_stream / generate_tokens_inner on token ids (mod.rs:137-238, 268-340): a stream of its own on the shared
// model -- fresh cache, seed-0 sampler, one callback per token; the callback returning 0 is the dropped receiver.
// Thread-safe for concurrent calls on one handle (each call owns its cache).
int flh_generate_stream(void *hv, const uint32_t *prompt, size_t T, size_t max_tokens, float temperature, int64_t eos,
                        int (*on_token)(uint32_t token, void *user), void *user, size_t *forwards) {
    return guard([&] {
        const Handle *h = static_cast<const Handle *>(hv);
        if (!on_token) throw Error(FL_ERR_BAD_ARGUMENT, "null token callback");
        std::vector<uint32_t> p(prompt, prompt + T);
        std::optional<uint32_t> e = eos >= 0 ? std::optional<uint32_t>((uint32_t)eos) : std::nullopt;
        auto cb = [&](uint32_t t) { return on_token(t, user) != 0; };
        size_t fw = 0;
        if (h->llama) fw = h->llama->generate_stream_ids(p, max_tokens, temperature, e, cb);
        else if (h->mistral) fw = h->mistral->generate_stream_ids(p, max_tokens, temperature, e, cb);
        else fw = h->qwen->generate_stream_ids(p, max_tokens, temperature, e, cb);
        if (forwards) *forwards = fw;
        return 0;
    });
}

// LogitsProcessor::new(seed, temperature, None) / .sample (mod.rs:373-374,425-428); has_temperature 0 = None
int flh_logits_processor_new(uint64_t seed, int has_temperature, double temperature, void **out) {
    return guard([&] {
        *out = new LogitsProcessor(seed, has_temperature ? std::optional<double>(temperature) : std::nullopt);
        return 0;
    });
}
int flh_logits_processor_sample(void *lp, const float *logits, size_t n, uint32_t *token_out, uint64_t *draws_out) {
    return guard([&] {
        LogitsProcessor *p = static_cast<LogitsProcessor *>(lp);
        *token_out = p->sample(logits, n);
        if (draws_out) *draws_out = p->draws();
        return 0;
    });
}
void flh_logits_processor_free(void *lp) { delete static_cast<LogitsProcessor *>(lp); }

// ModelInitializer::forward through the model's own cache object (trait-level call)
int flh_forward(void *hv, const uint32_t *ids, size_t T, size_t pos, float *logits_out, size_t *n_logits) {
    return guard([&] {
        Handle *h = static_cast<Handle *>(hv);
        Tensor in = Tensor::from_ids(std::vector<uint32_t>(ids, ids + T)), lg;
        if (h->llama) lg = h->llama->model.forward(in, pos, h->llama->cache);
        else if (h->mistral) lg = h->mistral->model.forward(in, pos, h->mistral->cache);
        else lg = h->qwen->model.forward(in, pos, h->qwen->cache);
        const size_t n = (size_t)lg.elem_count();
        std::memcpy(logits_out, lg.f32(), n * sizeof(float));
        if (n_logits) *n_logits = n;
        return 0;
    });
}

size_t flh_cache_offset(void *hv) {
    Handle *h = static_cast<Handle *>(hv);
    if (h->llama) return h->llama->cache.get_offset();
    if (h->mistral) return h->mistral->cache.get_offset();
    return h->qwen->cache.get_offset();
}

void flh_cache_reset(void *hv) {           // ModelCache::reset (+ a fresh cache object for Llama)
    Handle *h = static_cast<Handle *>(hv);
    if (h->llama) h->llama->cache = LlamaWithConfig::initialize_cache(h->llama->device, h->llama->dtype);
    else if (h->mistral) h->mistral->cache.reset();
    else h->qwen->cache.reset();
}

// StreamBatcher (fastllm_host.hpp): the reference's concurrent streams (mod.rs:137-238) on one batched decode loop
namespace {
struct BatcherHandle { std::unique_ptr<StreamBatcher> b; };
std::shared_ptr<detail::ModelHandle> model_of(Handle *h) {
    if (h->llama) return h->llama->model.model;
    if (h->mistral) return h->mistral->model.model;
    return h->qwen->model.model;
}
}  // namespace
int flh_batcher_create(void *hv, size_t slots, size_t max_seq, size_t chunk, void **out) {
    return guard([&] {
        if (!hv || !out) throw Error(FL_ERR_BAD_ARGUMENT, "null argument");
        auto bh = std::make_unique<BatcherHandle>();
        Handle *h = static_cast<Handle *>(hv);
        bh->b = std::make_unique<StreamBatcher>(model_of(h), slots, max_seq, chunk, !h->llama && pos_mode() == PosMode::Reference);
        *out = bh.release();
        return 0;
    });
}
// ... on an fl_model the caller already holds (a reference is taken): a host that built the model through the C ABI itself
int flh_batcher_create_on(void *fl_model_ptr, size_t slots, size_t max_seq, size_t chunk, int counter_positions, void **out) {
    return guard([&] {
        if (!fl_model_ptr || !out) throw Error(FL_ERR_BAD_ARGUMENT, "null argument");
        fl_model *m = static_cast<fl_model *>(fl_model_ptr);
        fl_model_retain(m);
        auto mh = std::make_shared<detail::ModelHandle>(m);          // (releases the reference)
        auto bh = std::make_unique<BatcherHandle>();
        bh->b = std::make_unique<StreamBatcher>(mh, slots, max_seq, chunk, counter_positions != 0);
        *out = bh.release();
        return 0;
    });
}
int flh_batcher_submit(void *bv, const uint32_t *prompt, size_t T, size_t max_tokens, float temperature, int64_t eos,
                       int (*on_token)(uint64_t id, uint32_t token, void *user), void (*on_done)(uint64_t id, size_t n_tokens, void *user),
                       void *user, uint64_t *id_out) {
    return guard([&] {
        if (!bv || !on_token || (!prompt && T)) throw Error(FL_ERR_BAD_ARGUMENT, "null argument");
        auto *bh = static_cast<BatcherHandle *>(bv);
        auto id = std::make_shared<uint64_t>(0);
        std::optional<uint32_t> e = eos >= 0 ? std::optional<uint32_t>((uint32_t)eos) : std::nullopt;
        StreamBatcher::OnDone done;
        if (on_done) done = [=](size_t n) { on_done(*id, n, user); };
        *id = bh->b->submit(std::vector<uint32_t>(prompt, prompt + T), max_tokens, temperature, e,
                            [=](uint32_t t) { return on_token(*id, t, user) != 0; }, done);
        if (id_out) *id_out = *id;
        return 0;
    });
}
// ... a request with logit rules of its own (StreamBatcher::submit with LogitRules), as flh_generate_rules takes them
int flh_batcher_submit_rules(void *bv, const uint32_t *prompt, size_t T, size_t max_tokens, float temperature, int64_t eos, size_t n_bias,
                             const uint32_t *bias_ids, const float *bias_values, float repetition_penalty, float frequency_penalty,
                             float presence_penalty, int (*on_token)(uint64_t id, uint32_t token, void *user),
                             void (*on_done)(uint64_t id, size_t n_tokens, void *user), void *user, uint64_t *id_out) {
    return guard([&] {
        if (!bv || !on_token || (!prompt && T) || (n_bias && (!bias_ids || !bias_values))) throw Error(FL_ERR_BAD_ARGUMENT, "null argument");
        auto *bh = static_cast<BatcherHandle *>(bv);
        auto id = std::make_shared<uint64_t>(0);
        std::optional<uint32_t> e = eos >= 0 ? std::optional<uint32_t>((uint32_t)eos) : std::nullopt;
        StreamBatcher::OnDone done;
        if (on_done) done = [=](size_t n) { on_done(*id, n, user); };
        *id = bh->b->submit(std::vector<uint32_t>(prompt, prompt + T), max_tokens, temperature, e, SamplingOptions{},
                            make_rules(n_bias, bias_ids, bias_values, repetition_penalty, frequency_penalty, presence_penalty),
                            [=](uint32_t t) { return on_token(*id, t, user) != 0; }, done);
        if (id_out) *id_out = *id;
        return 0;
    });
}
// ... a guided request (generate_ids with GuideOptions; stream != 0: generate_stream_ids' guided overload): the automaton as the CSR
// arrays of fl_guide_desc, start_state the state of the first token; top_p <= 0 and top_k <= 0: off
int flh_generate_guide(void *hv, const uint32_t *prompt, size_t T, size_t max_tokens, float temperature, int64_t eos, double top_p,
                       int64_t top_k, uint32_t n_states, const uint64_t *row_ptr, const uint32_t *tokens, const uint32_t *next,
                       uint32_t start_state, int stream, uint32_t *out_tokens, size_t *n_out) {
    return guard([&] {
        Handle *h = static_cast<Handle *>(hv);
        if (!h || !row_ptr || !tokens || !next || !out_tokens || !n_out) throw Error(FL_ERR_BAD_ARGUMENT, "null argument");
        std::vector<uint32_t> p(prompt, prompt + T), r;
        std::optional<uint32_t> e = eos >= 0 ? std::optional<uint32_t>((uint32_t)eos) : std::nullopt;
        SamplingOptions opt;
        if (top_p > 0) opt.top_p = top_p;
        if (top_k > 0) opt.top_k = (size_t)top_k;
        const size_t nnz = (size_t)row_ptr[n_states];
        GuideOptions g;
        g.guide = Guide(model_of(h)->m, std::vector<uint64_t>(row_ptr, row_ptr + n_states + 1), std::vector<uint32_t>(tokens, tokens + nnz),
                        std::vector<uint32_t>(next, next + nnz));
        g.start_state = start_state;
        if (stream) {
            auto on = [&](uint32_t t) { r.push_back(t); return true; };
            if (h->llama) h->llama->generate_stream_ids(p, max_tokens, temperature, e, opt, g, nullptr, on);
            else if (h->mistral) h->mistral->generate_stream_ids(p, max_tokens, temperature, e, opt, g, nullptr, on);
            else h->qwen->generate_stream_ids(p, max_tokens, temperature, e, opt, g, nullptr, on);
        } else if (h->llama) r = h->llama->generate_ids(p, max_tokens, temperature, e, opt, g);
        else if (h->mistral) r = h->mistral->generate_ids(p, max_tokens, temperature, e, opt, g);
        else r = h->qwen->generate_ids(p, max_tokens, temperature, e, opt, g);
        for (size_t i = 0; i < r.size(); i++) out_tokens[i] = r[i];
        *n_out = r.size();
        return 0;
    });
}
// ... a FULL request with prompt-lookup drafts (generate_ids / generate_stream_ids with LookupOptions + LogitRules + GuideOptions +
// top_logprobs): has_rules != 0: the n_bias pairs and the three penalties; n_states > 0: the automaton; top_logprobs < 0: no log-probs,
// else token_logprob [max_tokens] (and top_ids / top_lps [max_tokens][top_logprobs]) receive them; max_draft < 0: NO lookup -- the plain
// ruled, guided generate_ids, for comparison.  stats (optional): steps, drafted, accepted of the non-stream form.
int flh_generate_lookup_request(void *hv, const uint32_t *prompt, size_t T, size_t max_tokens, float temperature, int64_t eos, double top_p,
                                int64_t top_k, int has_rules, size_t n_bias, const uint32_t *bias_ids, const float *bias_values,
                                float repetition_penalty, float frequency_penalty, float presence_penalty, uint32_t n_states,
                                const uint64_t *row_ptr, const uint32_t *tokens, const uint32_t *next, uint32_t start_state, int max_draft,
                                int ngram_max, int ngram_min, int stream, int top_logprobs, uint32_t *out_tokens, size_t *n_out,
                                float *token_logprob, uint32_t *top_ids, float *top_lps, size_t *forwards, uint64_t stats[3]) {
    return guard([&] {
        Handle *h = static_cast<Handle *>(hv);
        if (!h || !prompt || !out_tokens || !n_out) throw Error(FL_ERR_BAD_ARGUMENT, "null argument");
        if (n_states > 0 && (!row_ptr || !tokens || !next)) throw Error(FL_ERR_BAD_ARGUMENT, "null guide arrays");
        if (top_logprobs >= 0 && !token_logprob) throw Error(FL_ERR_BAD_ARGUMENT, "null token_logprob");
        std::vector<uint32_t> p(prompt, prompt + T), r;
        std::optional<uint32_t> e = eos >= 0 ? std::optional<uint32_t>((uint32_t)eos) : std::nullopt;
        SamplingOptions opt;
        if (top_p > 0) opt.top_p = top_p;
        if (top_k > 0) opt.top_k = (size_t)top_k;
        LogitRules rules;
        if (has_rules) rules = make_rules(n_bias, bias_ids, bias_values, repetition_penalty, frequency_penalty, presence_penalty);
        GuideOptions g;
        if (n_states > 0) {
            const size_t nnz = (size_t)row_ptr[n_states];
            g.guide = Guide(model_of(h)->m, std::vector<uint64_t>(row_ptr, row_ptr + n_states + 1), std::vector<uint32_t>(tokens, tokens + nnz),
                            std::vector<uint32_t>(next, next + nnz));
            g.start_state = start_state;
        }
        const LogitRules *rp = has_rules ? &rules : nullptr;
        const GuideOptions *gp = n_states > 0 ? &g : nullptr;
        LookupOptions lk; lk.max_draft = max_draft; lk.ngram_max = ngram_max; lk.ngram_min = ngram_min;
        fl_spec_stats st{};
        TokenLogprobs lps;
        size_t fw = 0;
        auto run = [&](auto &m) {
            if (max_draft < 0) { r = m.generate_ids(p, max_tokens, temperature, e, opt, rp, gp); fw = m.forwards; }
            else if (stream) {
                const size_t w = top_logprobs > 0 ? (size_t)top_logprobs : 0;
                lps.top_n = (int)w;
                fw = m.generate_stream_ids(p, max_tokens, temperature, e, opt, lk, rp, gp, [&](uint32_t t) { r.push_back(t); return true; }, top_logprobs,
                                           [&](float v, const uint32_t *ids, const float *vals) {
                                               lps.token.push_back(v);
                                               lps.top_ids.insert(lps.top_ids.end(), ids, ids + w);
                                               lps.top.insert(lps.top.end(), vals, vals + w);
                                           });
            } else { r = m.generate_ids(p, max_tokens, temperature, e, opt, lk, rp, gp, top_logprobs, top_logprobs >= 0 ? &lps : nullptr, &st); fw = m.forwards; }
        };
        if (h->llama) run(*h->llama);
        else if (h->mistral) run(*h->mistral);
        else run(*h->qwen);
        for (size_t i = 0; i < r.size(); i++) out_tokens[i] = r[i];
        *n_out = r.size();
        if (top_logprobs >= 0 && max_draft >= 0) {
            for (size_t i = 0; i < lps.token.size(); i++) token_logprob[i] = lps.token[i];
            if (top_ids) for (size_t i = 0; i < lps.top_ids.size(); i++) top_ids[i] = lps.top_ids[i];
            if (top_lps) for (size_t i = 0; i < lps.top.size(); i++) top_lps[i] = lps.top[i];
        }
        if (forwards) *forwards = fw;
        if (stats) { stats[0] = st.steps; stats[1] = st.drafted; stats[2] = st.accepted; }
        return 0;
    });
}
// ... a request with a guide of its own (StreamBatcher::submit with GuideOptions); hv: the model the batcher was made for
int flh_batcher_submit_guide(void *bv, void *hv, const uint32_t *prompt, size_t T, size_t max_tokens, float temperature, int64_t eos,
                             uint32_t n_states, const uint64_t *row_ptr, const uint32_t *tokens, const uint32_t *next, uint32_t start_state,
                             int (*on_token)(uint64_t id, uint32_t token, void *user), void (*on_done)(uint64_t id, size_t n_tokens, void *user),
                             void *user, uint64_t *id_out) {
    return guard([&] {
        if (!bv || !hv || !on_token || (!prompt && T) || !row_ptr || !tokens || !next) throw Error(FL_ERR_BAD_ARGUMENT, "null argument");
        auto *bh = static_cast<BatcherHandle *>(bv);
        auto id = std::make_shared<uint64_t>(0);
        std::optional<uint32_t> e = eos >= 0 ? std::optional<uint32_t>((uint32_t)eos) : std::nullopt;
        const size_t nnz = (size_t)row_ptr[n_states];
        GuideOptions g;
        g.guide = Guide(model_of(static_cast<Handle *>(hv))->m, std::vector<uint64_t>(row_ptr, row_ptr + n_states + 1),
                        std::vector<uint32_t>(tokens, tokens + nnz), std::vector<uint32_t>(next, next + nnz));
        g.start_state = start_state;
        StreamBatcher::OnDone done;
        if (on_done) done = [=](size_t n) { on_done(*id, n, user); };
        *id = bh->b->submit(std::vector<uint32_t>(prompt, prompt + T), max_tokens, temperature, e, SamplingOptions{}, std::nullopt, g,
                            [=](uint32_t t) { return on_token(*id, t, user) != 0; }, done);
        if (id_out) *id_out = *id;
        return 0;
    });
}
int flh_batcher_run(void *bv, size_t *batch_steps, size_t *prefills) {
    return guard([&] {
        if (!bv) throw Error(FL_ERR_BAD_ARGUMENT, "null argument");
        auto *bh = static_cast<BatcherHandle *>(bv);
        bh->b->run();
        if (batch_steps) *batch_steps = bh->b->batch_steps;
        if (prefills) *prefills = bh->b->prefills;
        return 0;
    });
}
void flh_batcher_destroy(void *bv) { delete static_cast<BatcherHandle *>(bv); }

// ... with a PrefixStore of `entries` caches (PrefixOptions; entries == 0: flh_batcher_create).  The position mode is flh_batcher_create's:
// a Mistral / Qwen2 model under FASTLLM_POS_MODE=reference asks for call-counter positions, which a store refuses (FL_ERR_BAD_ARGUMENT).
int flh_batcher_create_prefix(void *hv, size_t slots, size_t max_seq, size_t chunk, size_t entries, size_t min_match, void **out) {
    return guard([&] {
        if (!hv || !out) throw Error(FL_ERR_BAD_ARGUMENT, "null argument");
        auto bh = std::make_unique<BatcherHandle>();
        Handle *h = static_cast<Handle *>(hv);
        PrefixOptions po; po.entries = entries; po.min_match = min_match;
        bh->b = std::make_unique<StreamBatcher>(model_of(h), slots, max_seq, chunk, !h->llama && pos_mode() == PosMode::Reference, po);
        *out = bh.release();
        return 0;
    });
}
int flh_batcher_prefix_stats(void *bv, size_t *prefix_hits, size_t *prefix_tokens_reused, size_t *prefill_tokens) {
    return guard([&] {
        if (!bv) throw Error(FL_ERR_BAD_ARGUMENT, "null argument");
        auto *bh = static_cast<BatcherHandle *>(bv);
        if (prefix_hits) *prefix_hits = bh->b->prefix_hits;
        if (prefix_tokens_reused) *prefix_tokens_reused = bh->b->prefix_tokens_reused;
        if (prefill_tokens) *prefill_tokens = bh->b->prefill_tokens;
        return 0;
    });
}

// ... and with PackedAdmit (the admissions of one step share fl_batch_prefill calls): flh_batcher_create_prefix plus the three option
// values; packed_on == 0 is flh_batcher_create_prefix
int flh_batcher_create_packed(void *hv, size_t slots, size_t max_seq, size_t chunk, size_t entries, size_t min_match, int packed_on,
                              size_t max_prompt, size_t max_tokens, void **out) {
    return guard([&] {
        if (!hv || !out) throw Error(FL_ERR_BAD_ARGUMENT, "null argument");
        auto bh = std::make_unique<BatcherHandle>();
        Handle *h = static_cast<Handle *>(hv);
        PrefixOptions po; po.entries = entries; po.min_match = min_match;
        PackedAdmit pa; pa.on = packed_on != 0; pa.max_prompt = max_prompt; pa.max_tokens = max_tokens;
        bh->b = std::make_unique<StreamBatcher>(model_of(h), slots, max_seq, chunk, !h->llama && pos_mode() == PosMode::Reference, po, pa);
        *out = bh.release();
        return 0;
    });
}
// ... on an fl_model the caller already holds (flh_batcher_create_on), no store
int flh_batcher_create_on_packed(void *fl_model_ptr, size_t slots, size_t max_seq, size_t chunk, int counter_positions, int packed_on,
                                 size_t max_prompt, size_t max_tokens, void **out) {
    return guard([&] {
        if (!fl_model_ptr || !out) throw Error(FL_ERR_BAD_ARGUMENT, "null argument");
        fl_model *m = static_cast<fl_model *>(fl_model_ptr);
        fl_model_retain(m);
        auto mh = std::make_shared<detail::ModelHandle>(m);          // (releases the reference)
        auto bh = std::make_unique<BatcherHandle>();
        PackedAdmit pa; pa.on = packed_on != 0; pa.max_prompt = max_prompt; pa.max_tokens = max_tokens;
        bh->b = std::make_unique<StreamBatcher>(mh, slots, max_seq, chunk, counter_positions != 0, PrefixOptions{}, pa);
        *out = bh.release();
        return 0;
    });
}
// ... with BatchLookup (a step with drafts is one fl_batch_verify over the active slots): flh_batcher_create_on plus the option's values;
// lookup_on == 0 is flh_batcher_create_on
int flh_batcher_create_on_lookup(void *fl_model_ptr, size_t slots, size_t max_seq, size_t chunk, int counter_positions, int lookup_on, int max_draft,
                                 int ngram_max, int ngram_min, size_t min_drafted, void **out) {
    return guard([&] {
        if (!fl_model_ptr || !out) throw Error(FL_ERR_BAD_ARGUMENT, "null argument");
        fl_model *m = static_cast<fl_model *>(fl_model_ptr);
        fl_model_retain(m);
        auto mh = std::make_shared<detail::ModelHandle>(m);          // (releases the reference)
        auto bh = std::make_unique<BatcherHandle>();
        BatchLookup bl; bl.on = lookup_on != 0; bl.lookup.max_draft = max_draft; bl.lookup.ngram_max = ngram_max; bl.lookup.ngram_min = ngram_min;
        bl.min_drafted = min_drafted;
        bh->b = std::make_unique<StreamBatcher>(mh, slots, max_seq, chunk, counter_positions != 0, PrefixOptions{}, PackedAdmit{}, bl);
        *out = bh.release();
        return 0;
    });
}
// packed verify steps the batcher ran, and the ids drafted / accepted in them
int flh_batcher_lookup_stats(void *bv, size_t *verify_steps, size_t *drafted, size_t *accepted) {
    return guard([&] {
        if (!bv) throw Error(FL_ERR_BAD_ARGUMENT, "null argument");
        auto *bh = static_cast<BatcherHandle *>(bv);
        if (verify_steps) *verify_steps = bh->b->verify_steps;
        if (drafted) *drafted = bh->b->drafted;
        if (accepted) *accepted = bh->b->accepted;
        return 0;
    });
}
// forwards the admissions took, and how many of them were packed calls
int flh_batcher_packed_stats(void *bv, size_t *prefill_calls, size_t *packed_calls) {
    return guard([&] {
        if (!bv) throw Error(FL_ERR_BAD_ARGUMENT, "null argument");
        auto *bh = static_cast<BatcherHandle *>(bv);
        if (prefill_calls) *prefill_calls = bh->b->prefill_calls;
        if (packed_calls) *packed_calls = bh->b->packed_calls;
        return 0;
    });
}

// PrefixIndex alone (pure host, no GPU).  entry_out: the entry, or -1 (match: a miss; insert: nothing stored)
int flh_prefix_index_create(size_t entries, void **out) {
    return guard([&] {
        if (!out) throw Error(FL_ERR_BAD_ARGUMENT, "null argument");
        *out = new PrefixIndex(entries);
        return 0;
    });
}
int flh_prefix_index_match(void *pv, const uint32_t *prompt, size_t n_prompt, size_t min_match, int64_t *entry_out, size_t *n_out) {
    return guard([&] {
        if (!pv || !entry_out || !n_out || (!prompt && n_prompt)) throw Error(FL_ERR_BAD_ARGUMENT, "null argument");
        auto r = static_cast<PrefixIndex *>(pv)->match(std::vector<uint32_t>(prompt, prompt + n_prompt), min_match);
        *entry_out = r.first == PrefixIndex::npos ? -1 : (int64_t)r.first;
        *n_out = r.second;
        return 0;
    });
}
int flh_prefix_index_insert(void *pv, const uint32_t *ids, size_t n_ids, int64_t *entry_out) {
    return guard([&] {
        if (!pv || !entry_out || (!ids && n_ids)) throw Error(FL_ERR_BAD_ARGUMENT, "null argument");
        const size_t e = static_cast<PrefixIndex *>(pv)->insert(std::vector<uint32_t>(ids, ids + n_ids));
        *entry_out = e == PrefixIndex::npos ? -1 : (int64_t)e;
        return 0;
    });
}
void flh_prefix_index_destroy(void *pv) { delete static_cast<PrefixIndex *>(pv); }

// EmbeddingModel (fastllm_host.hpp): the reference's embeddings trait (embeddings.rs:17-38) on token ids
int flh_embedding_create(const char *config_json, const fl_tensor *tensors, size_t n, int dtype, int device_ordinal, int activation,
                         int add_token_type0, void **out) {
    return guard([&] {
        if (!config_json || !out) throw Error(FL_ERR_BAD_ARGUMENT, "null argument");
        const BertConfig cfg = BertConfig::from_json(config_json);
        EmbeddingOptions opt; opt.activation = (fl_activation)activation; opt.add_token_type0 = add_token_type0 != 0;
        const Device dev = device_ordinal < 0 ? Device::cpu() : Device::mi355x(device_ordinal);
        *out = new EmbeddingModel(cfg, to_map(tensors, n), (DType)dtype, dev, "synthetic", opt);
        return 0;
    });
}
void flh_embedding_destroy(void *ev) { delete static_cast<EmbeddingModel *>(ev); }
size_t flh_embedding_size(void *ev) { return static_cast<EmbeddingModel *>(ev)->embedding_size(); }
int flh_embed_ids(void *ev, const uint32_t *ids, size_t T, float *out, size_t *token_count) {
    return guard([&] {
        if (!ev || !out) throw Error(FL_ERR_BAD_ARGUMENT, "null argument");
        const EmbeddingOutput r = static_cast<EmbeddingModel *>(ev)->embed_ids(std::vector<uint32_t>(ids, ids + T));
        std::memcpy(out, r.embeddings.data(), r.embeddings.size() * sizeof(float));
        if (token_count) *token_count = r.token_count;
        return 0;
    });
}
int flh_embed_batch_ids(void *ev, const uint32_t *ids, const size_t *offsets, size_t n_seq, float *out) {
    return guard([&] {
        if (!ev || !out || !offsets) throw Error(FL_ERR_BAD_ARGUMENT, "null argument");
        std::vector<std::vector<uint32_t>> seqs;
        for (size_t s = 0; s < n_seq; s++) seqs.emplace_back(ids + offsets[s], ids + offsets[s + 1]);
        const auto *em = static_cast<EmbeddingModel *>(ev);
        const std::vector<EmbeddingOutput> r = em->embed_batch_ids(seqs);
        for (size_t s = 0; s < n_seq; s++) std::memcpy(out + s * em->embedding_size(), r[s].embeddings.data(), em->embedding_size() * sizeof(float));
        return 0;
    });
}
int flh_compute_similarity_ids(void *ev, const uint32_t *a, size_t na, const uint32_t *b, size_t nb, float *out) {
    return guard([&] {
        if (!ev || !out) throw Error(FL_ERR_BAD_ARGUMENT, "null argument");
        *out = static_cast<EmbeddingModel *>(ev)->compute_similarity_ids(std::vector<uint32_t>(a, a + na), std::vector<uint32_t>(b, b + nb));
        return 0;
    });
}

// DecoderEmbeddingModel (fastllm_host.hpp): the same surface over an fl_model the caller already holds (a reference is taken)
int flh_decoder_embedding_create_on(void *fl_model_ptr, int pooling, int mask, int normalize, size_t dimensions, size_t slots, size_t max_seq,
                                    void **out) {
    return guard([&] {
        if (!fl_model_ptr || !out) throw Error(FL_ERR_BAD_ARGUMENT, "null argument");
        fl_model *m = static_cast<fl_model *>(fl_model_ptr);
        fl_model_retain(m);
        auto mh = std::make_shared<detail::ModelHandle>(m);          // (releases the reference)
        DecoderEmbeddingOptions opt;
        opt.pooling = (fl_pooling)pooling; opt.mask = (fl_attn_mask)mask; opt.normalize = normalize != 0;
        opt.dimensions = dimensions; opt.slots = slots; opt.max_seq = max_seq;
        *out = new DecoderEmbeddingModel(mh, opt, "synthetic");
        return 0;
    });
}
void flh_decoder_embedding_destroy(void *ev) { delete static_cast<DecoderEmbeddingModel *>(ev); }
size_t flh_decoder_embedding_size(void *ev) { return static_cast<DecoderEmbeddingModel *>(ev)->embedding_size(); }
size_t flh_decoder_embedding_calls(void *ev) { return static_cast<DecoderEmbeddingModel *>(ev)->calls(); }
int flh_decoder_embed_batch_ids(void *ev, const uint32_t *ids, const size_t *offsets, size_t n_seq, float *out) {
    return guard([&] {
        if (!ev || !out || !offsets) throw Error(FL_ERR_BAD_ARGUMENT, "null argument");
        std::vector<std::vector<uint32_t>> seqs;
        for (size_t s = 0; s < n_seq; s++) seqs.emplace_back(ids + offsets[s], ids + offsets[s + 1]);
        auto *em = static_cast<DecoderEmbeddingModel *>(ev);
        const std::vector<EmbeddingOutput> r = em->embed_batch_ids(seqs);
        for (size_t s = 0; s < n_seq; s++) std::memcpy(out + s * em->embedding_size(), r[s].embeddings.data(), em->embedding_size() * sizeof(float));
        return 0;
    });
}
int flh_decoder_embed_ids(void *ev, const uint32_t *ids, size_t T, float *out, size_t *token_count) {
    return guard([&] {
        if (!ev || !out) throw Error(FL_ERR_BAD_ARGUMENT, "null argument");
        const EmbeddingOutput r = static_cast<DecoderEmbeddingModel *>(ev)->embed_ids(std::vector<uint32_t>(ids, ids + T));
        std::memcpy(out, r.embeddings.data(), r.embeddings.size() * sizeof(float));
        if (token_count) *token_count = r.token_count;
        return 0;
    });
}
int flh_decoder_compute_similarity_ids(void *ev, const uint32_t *a, size_t na, const uint32_t *b, size_t nb, float *out) {
    return guard([&] {
        if (!ev || !out) throw Error(FL_ERR_BAD_ARGUMENT, "null argument");
        *out = static_cast<DecoderEmbeddingModel *>(ev)->compute_similarity_ids(std::vector<uint32_t>(a, a + na), std::vector<uint32_t>(b, b + nb));
        return 0;
    });
}

}  // extern "C"
