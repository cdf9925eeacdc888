// encoder.h -- the fl_encoder object behind the C ABI: the BERT / MiniLM encoder forward (the reference's MiniLMModel,
// src/models/embeddings.rs) on one GPU.
#pragma once
#include <mutex>
#include <vector>

#include "kernels.h"

namespace fl {

struct EncLayerW {
    void *wqkv = nullptr;        // [3h, h]  query | key | value rows (compute dtype)
    float *bqkv = nullptr;       // [3h]
    void *wo = nullptr;          // [h, h]   attention.output.dense
    float *bo = nullptr;
    float *ln1w = nullptr, *ln1b = nullptr;   // attention.output.LayerNorm
    void *wi = nullptr;          // [I, h]   intermediate.dense
    float *bi = nullptr;
    void *wout = nullptr;        // [h, I]   output.dense
    float *bout = nullptr;
    float *ln2w = nullptr, *ln2b = nullptr;   // output.LayerNorm
};

struct Encoder {
    std::mutex mu;               // submission is serialised per encoder
    int device = 0, dtype = FL_DTYPE_BF16, act = ENC_ACT_GELU_TANH;
    int64_t h = 0, inter = 0, L = 0, H = 0, d = 0, P = 0, V = 0, max_T = 0;
    float eps = 0.f;
    hipStream_t stream = nullptr;
    void *word = nullptr, *pos = nullptr, *tt0 = nullptr;     // [V,h] | [P,h] | [h] (add_token_type0) in the compute dtype
    float *lnw = nullptr, *lnb = nullptr;                     // embeddings.LayerNorm
    std::vector<EncLayerW> layers;
    // workspace, sized once from max_batch_tokens
    int64_t slab_rows = 0;       // rows of `y`: every call's T x (K slabs the planner may leave at T)
    float *x_res = nullptr;      // [T][h] fp32 residual stream
    void *xn = nullptr;          // [T][h] its compute-dtype copy (the next projection's input)
    float *y = nullptr;          // [slab_rows][max(3h, I)] fp32 projection output, split-K slabs
    void *qkv = nullptr;         // [T][3h] compute dtype
    void *ao = nullptr;          // [T][h] attention output
    void *gelu = nullptr;        // [T][I]
    float *pooled = nullptr;     // [n_seq][h]
    uint32_t *ids = nullptr;     // [T]
    int32_t *row_seq = nullptr, *offsets = nullptr;           // [T] | [T + 1]
    int64_t hbm_bytes = 0;
    std::vector<void *> allocs;
    size_t esize() const { return dtype == FL_DTYPE_BF16 ? 2 : 4; }
    ~Encoder();
};

int encoder_create(const fl_encoder_config *cfg, const fl_tensor *tensors, size_t n, int compute_dtype, int device, Encoder **out);
// hidden_out [T][h] (one sequence: n_seq == 1) or embed_out [n_seq][h]; exactly one of the two is non-null
int encoder_run(Encoder *e, const uint32_t *ids, const size_t *offsets, size_t n_seq, float *hidden_out, float *embed_out);
// fl_op_encoder_attention: the shape / offsets checks shared with the op (FL_OK, or the error with the message set)
int encoder_check_offsets(const size_t *offsets, size_t n_seq, int64_t max_len, int64_t max_total, int64_t *total_out, int64_t *longest_out);

}  // namespace fl
