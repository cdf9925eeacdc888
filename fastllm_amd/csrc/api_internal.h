// api_internal.h -- what the two files of the extern "C" surface (api.hip, api_ops.hip) share: the exception barrier, the handle
// casts and the older sampler struct widened.
#pragma once
#include <exception>
#include <new>

#include "model.h"

namespace fl {

// fl_model / fl_cache stay opaque: the handles are the C++ objects themselves
inline Model *M(fl_model *m) { return reinterpret_cast<Model *>(m); }
inline const Model *M(const fl_model *m) { return reinterpret_cast<const Model *>(m); }
inline Cache *C(fl_cache *c) { return reinterpret_cast<Cache *>(c); }
inline const Cache *C(const fl_cache *c) { return reinterpret_cast<const Cache *>(c); }

template <typename F> int guarded(F &&body) noexcept {
    try {
        return body();
    } catch (const std::bad_alloc &) {
        set_error("out of host memory (std::bad_alloc)");
        return FL_ERR_OOM;
    } catch (const std::exception &e) {
        set_error("internal error: %s", e.what());
        return FL_ERR_HIP;
    } catch (...) {
        set_error("internal error: unknown C++ exception");
        return FL_ERR_HIP;
    }
}
template <typename F> void guarded_void(F &&body) noexcept {
    (void)guarded([&]() -> int { body(); return FL_OK; });
}

// the older sampler struct as the one every path takes: no top_p, no top_k
inline fl_sampler widen(const fl_sampling &sp) {
    fl_sampler s{};
    s.struct_size = sizeof(fl_sampler);
    s.temperature = sp.temperature; s.seed = sp.seed; s.draws_done = sp.draws_done;
    return s;
}

}  // namespace fl
