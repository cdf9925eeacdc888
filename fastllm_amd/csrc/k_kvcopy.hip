// k_kvcopy.hip -- the first n cached positions of one KV cache into another cache of the same model (fl_cache_copy_prefix).
//
// Two caches of one model differ only in seq_alloc, so for each of K and V the prefix is a 2-D byte copy: `rows` rows of `width`
// bytes, with a source and a destination pitch (K and row-major V: L*Hkvs rows of n*d*es bytes; transposed V: L*Hkvs*d rows of
// n*es bytes).  ONE launch takes both tensors and every layer.
//
// Lane mapping: the unit of work is a 16-byte chunk of a row, numbered row-major over job A and then job B; consecutive lanes take
// consecutive chunks.  A long row (K: tens of KB) is read and written as whole coalesced 1 KiB wave accesses; a short row (V^T at
// small n: a few hundred bytes, tens of thousands of rows) still fills every lane of a wave, because a wave simply runs on into the
// next rows -- a workgroup per row would leave most of its lanes idle.  The grid is sized to the chip (kBlocksPerCu workgroups per
// CU), not to the row count; every thread walks the chunk numbers with the grid's stride, kUnroll chunks per pass with all loads of
// a pass issued before its stores (the copy is latency-bound per lane, so the independent loads are what fills the memory system).
//
// Bytes: a row's last chunk may hold 2 ... 14 bytes (width is a multiple of 2: V^T rows are 2n bytes).  It is moved as an 8-, a 4-
// and a 2-byte piece as the bits of its length say, so exactly the bytes [0, width) of every destination row are written and exactly
// those of every source row are read (a row may end where its allocation ends: pitch == width on the last row).  Row starts are
// 16-byte aligned on both sides (pitches are multiples of 16, the bases come from the allocator), so every piece is naturally aligned.
#include <algorithm>

#include "kernels.h"

namespace fl {

constexpr int kKvCopyThreads = 256;
constexpr int kKvCopyUnroll = 4;
constexpr int kKvCopyBlocksPerCu = 8;

struct KvCopyDev {                      // a job as the kernel reads it
    const char *src; char *dst;
    long long spitch, dpitch;
    unsigned long long chunks;          // rows * cpr
    unsigned cpr;                       // 16-byte chunks per row, the partial last one included
    unsigned width;                     // bytes per row
};

// compiler vector types (HIP's uint4 is a class and cannot live behind an address-space pointer).  The destination is global memory
// by construction; that is said in the pointer type so that the stores are global_store_*, not flat_store_*.
typedef uint32_t kv_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t kv_u32x2 __attribute__((ext_vector_type(2)));
#define KV_GLOBAL(T, p) ((__attribute__((address_space(1))) T *)(p))

__device__ __forceinline__ kv_u32x4 kv_load_chunk(const char *p, unsigned nb) {
    if (nb >= 16) return *KV_GLOBAL(const kv_u32x4, p);
    kv_u32x4 v = {0, 0, 0, 0};
    unsigned o = 0;
    if (nb & 8) { const kv_u32x2 t = *KV_GLOBAL(const kv_u32x2, p); v.x = t.x; v.y = t.y; o = 8; }
    if (nb & 4) { v.z = *KV_GLOBAL(const uint32_t, p + o); o += 4; }
    if (nb & 2) v.w = *KV_GLOBAL(const uint16_t, p + o);
    return v;
}

__device__ __forceinline__ void kv_store_chunk(char *p, unsigned nb, const kv_u32x4 &v) {
    if (nb >= 16) { *KV_GLOBAL(kv_u32x4, p) = v; return; }
    unsigned o = 0;
    if (nb & 8) { const kv_u32x2 t = {v.x, v.y}; *KV_GLOBAL(kv_u32x2, p) = t; o = 8; }
    if (nb & 4) { *KV_GLOBAL(uint32_t, p + o) = v.z; o += 4; }
    if (nb & 2) *KV_GLOBAL(uint16_t, p + o) = (uint16_t)v.w;
}

// IdxT: unsigned when the chunk count of both jobs together fits 32 bits (every cache there is), else unsigned long long
template <typename IdxT>
__global__ __launch_bounds__(kKvCopyThreads) void kv_copy_kernel(KvCopyDev a, KvCopyDev b) {
    const IdxT na = (IdxT)a.chunks, total = (IdxT)(a.chunks + b.chunks);
    const IdxT stride = (IdxT)gridDim.x * kKvCopyThreads;
    const IdxT first = (IdxT)blockIdx.x * kKvCopyThreads + threadIdx.x;
    // the last pass of a thread may start below `total` and end above it; i + u * stride cannot wrap: the host keeps
    // total + kKvCopyUnroll * stride inside IdxT
    for (IdxT i = first; i < total; i += stride * kKvCopyUnroll) {
        kv_u32x4 v[kKvCopyUnroll];
        char *dp[kKvCopyUnroll];
        unsigned nb[kKvCopyUnroll];
#pragma unroll
        for (int u = 0; u < kKvCopyUnroll; u++) {
            const IdxT idx = i + (IdxT)u * stride;
            nb[u] = 0;
            if (idx < total) {
                const bool in_a = idx < na;
                const IdxT k = in_a ? idx : idx - na;
                const IdxT cpr = (IdxT)(in_a ? a.cpr : b.cpr);
                const IdxT row = k / cpr;
                const unsigned off = (unsigned)(k - row * cpr) * 16u;
                nb[u] = min(16u, (in_a ? a.width : b.width) - off);
                dp[u] = (in_a ? a.dst : b.dst) + (long long)row * (in_a ? a.dpitch : b.dpitch) + off;
                v[u] = kv_load_chunk((in_a ? a.src : b.src) + (long long)row * (in_a ? a.spitch : b.spitch) + off, nb[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < kKvCopyUnroll; u++)
            if (nb[u]) kv_store_chunk(dp[u], nb[u], v[u]);
    }
}

int kv_copy_check(const KvCopyJob &j) {
    if (j.rows < 0 || j.width < 0 || (j.width & 1)) FL_FAIL(FL_ERR_BAD_ARGUMENT, "kv copy: rows and width must be >= 0 and width a multiple of 2 (got %lld rows of %lld bytes)", (long long)j.rows, (long long)j.width);
    if (j.width > (int64_t)0xfffffff0u) FL_FAIL(FL_ERR_BAD_ARGUMENT, "kv copy: a row of %lld bytes is too long", (long long)j.width);
    if ((j.spitch & 15) || (j.dpitch & 15) || j.spitch < j.width || j.dpitch < j.width)
        FL_FAIL(FL_ERR_BAD_ARGUMENT, "kv copy: pitches must be multiples of 16 and at least the width (%lld -> %lld, width %lld)", (long long)j.spitch, (long long)j.dpitch, (long long)j.width);
    return FL_OK;
}

static int kv_copy_check_buffers(const KvCopyJob &j) {
    if (j.rows == 0 || j.width == 0) return FL_OK;
    if (!j.src || !j.dst) FL_FAIL(FL_ERR_BAD_ARGUMENT, "kv copy: null buffer");
    if (((uintptr_t)j.src | (uintptr_t)j.dst) & 15) FL_FAIL(FL_ERR_BAD_ARGUMENT, "kv copy: buffers must be 16-byte aligned");
    return FL_OK;
}

int launch_kv_copy(Launcher &L, const KvCopyJob &ja, const KvCopyJob &jb) {
    FL_TRY(kv_copy_check(ja));
    FL_TRY(kv_copy_check(jb));
    FL_TRY(kv_copy_check_buffers(ja));
    FL_TRY(kv_copy_check_buffers(jb));
    auto dev = [](const KvCopyJob &j) {
        KvCopyDev d{};
        d.src = (const char *)j.src; d.dst = (char *)j.dst; d.spitch = j.spitch; d.dpitch = j.dpitch;
        d.width = (unsigned)j.width;
        d.cpr = (unsigned)((j.width + 15) / 16);
        d.chunks = (unsigned long long)j.rows * d.cpr;
        if (d.chunks == 0) d.cpr = 1;                 // (never divided by: the job has no chunk)
        return d;
    };
    const KvCopyDev a = dev(ja), b = dev(jb);
    const unsigned long long total = a.chunks + b.chunks;
    if (total == 0) return FL_OK;
    const unsigned long long per_pass = (unsigned long long)kKvCopyThreads * kKvCopyUnroll;
    const unsigned grid = (unsigned)std::min<unsigned long long>((total + per_pass - 1) / per_pass, (unsigned long long)device_cu_count() * kKvCopyBlocksPerCu);
    const double bytes = 2.0 * ((double)ja.rows * (double)ja.width + (double)jb.rows * (double)jb.width);     // read + write
    // 32-bit chunk numbers while a whole extra pass beyond `total` still fits (the loop's i + u * stride)
    if (total + (unsigned long long)grid * per_pass < 0xffffffffull)
        return L.launch(KC_KVCOPY, bytes, 0, kv_copy_kernel<unsigned>, dim3(grid), dim3(kKvCopyThreads), 0, a, b);
    return L.launch(KC_KVCOPY, bytes, 0, kv_copy_kernel<unsigned long long>, dim3(grid), dim3(kKvCopyThreads), 0, a, b);
}

}  // namespace fl
