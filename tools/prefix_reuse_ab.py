"""K/V prefix reuse, measured inside ONE process with the samples interleaved and medians reported (tools/prefill_ab.py's method).

1. Copy rate: the copy kernel (fl_op_kv_copy, k_kvcopy.hip) at the shapes of one Mistral-7B bf16 cache of capacity 4096 -- K: 256 rows
   of n * 256 bytes at a 1 MiB pitch; V^T: 32 768 rows of n * 2 bytes at an 8 KiB pitch -- for n = 128, 512, 2048, 4096, beside the
   same two copies as hipMemcpy2DAsync calls.  GB/s counts the bytes read plus the bytes written.  Both sides rotate over buffer
   pairs that together exceed the Infinity Cache.
2. Time to first token: synthetic Mistral-7B bf16 (as bench.py builds it), prompts of 512 + 32 and 2048 + 32 tokens:
   (a) fl_forward of the whole prompt on a fresh cache; (b) fl_cache_copy_prefix of the first 512 / 2048 positions from a cache that
   holds them, then fl_forward of the 32-token suffix.

usage: prefix_reuse_ab.py [copy] [ttft]     (default: both)"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (its HIP runtime must initialise before the product library's)
torch.cuda.is_available()
import bench  # noqa: E402
import fastllm_amd as fa  # noqa: E402
from fastllm_amd.configs import MODEL_CONFIGS  # noqa: E402

REPS = 7
what = set(sys.argv[1:]) or {"copy", "ttft"}


def med(xs):
    return float(np.median(xs)), float(min(xs)), float(max(xs))


class Hip:
    """The few runtime calls the hipMemcpy2DAsync side needs, from the runtime the product library is linked against."""

    def __init__(self):
        fa.lib()
        self.l = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
        vp, sz = C.c_void_p, C.c_size_t
        self.l.hipMalloc.argtypes = [C.POINTER(vp), sz]
        self.l.hipFree.argtypes = [vp]
        self.l.hipMemset.argtypes = [vp, C.c_int, sz]
        self.l.hipStreamCreate.argtypes = [C.POINTER(vp)]
        self.l.hipStreamSynchronize.argtypes = [vp]
        self.l.hipEventCreate.argtypes = [C.POINTER(vp)]
        self.l.hipEventRecord.argtypes = [vp, vp]
        self.l.hipEventSynchronize.argtypes = [vp]
        self.l.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), vp, vp]
        self.l.hipMemcpy2DAsync.argtypes = [vp, sz, vp, sz, sz, sz, C.c_int, vp]

    def ok(self, rc, what_):
        if rc != 0:
            raise RuntimeError("%s failed: hipError %d" % (what_, rc))

    def malloc(self, n):
        p = C.c_void_p()
        self.ok(self.l.hipMalloc(C.byref(p), n), "hipMalloc")
        self.ok(self.l.hipMemset(p, 1, n), "hipMemset")
        return p


def copy_rate():
    hip = Hip()
    L, Hkv, d, es, cap = 32, 8, 128, 2, 4096
    shapes = {"K": (L * Hkv, lambda n: n * d * es, cap * d * es), "Vt": (L * Hkv * d, lambda n: n * es, cap * es)}
    ncopy, iters = 2, 10                                  # 2 x (256 + 256) MiB per tensor: past the 256 MiB Infinity Cache
    bufs = {k: [(hip.malloc(r * p), hip.malloc(r * p)) for _ in range(ncopy)] for k, (r, _w, p) in shapes.items()}
    st, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    hip.ok(hip.l.hipStreamCreate(C.byref(st)), "hipStreamCreate")
    hip.ok(hip.l.hipEventCreate(C.byref(e0)), "hipEventCreate")
    hip.ok(hip.l.hipEventCreate(C.byref(e1)), "hipEventCreate")
    host = {k: (np.ones((r, p), np.uint8), np.zeros((r, p), np.uint8)) for k, (r, _w, p) in shapes.items()}

    def runtime_ms(n):
        def once(i):
            for k, (r, w, p) in shapes.items():
                s, dd = bufs[k][i % ncopy]
                hip.ok(hip.l.hipMemcpy2DAsync(dd, p, s, p, w(n), r, 3, st), "hipMemcpy2DAsync")     # 3: hipMemcpyDeviceToDevice
        for i in range(ncopy):
            once(i)
        hip.ok(hip.l.hipStreamSynchronize(st), "hipStreamSynchronize")
        hip.ok(hip.l.hipEventRecord(e0, st), "hipEventRecord")
        for i in range(iters):
            once(i)
        hip.ok(hip.l.hipEventRecord(e1, st), "hipEventRecord")
        hip.ok(hip.l.hipEventSynchronize(e1), "hipEventSynchronize")
        ms = C.c_float(0)
        hip.ok(hip.l.hipEventElapsedTime(C.byref(ms), e0, e1), "hipEventElapsedTime")
        return ms.value / iters

    def kernel_ms(n):                                     # K and V^T as two launches (a cache copy is ONE launch over both)
        return sum(fa.op_kv_copy(host[k][0], host[k][1], w(n), iters=iters)[1] for k, (_r, w, _p) in shapes.items())

    print("# copy rate, Mistral-7B bf16 cache shapes (capacity 4096), GB/s = (read + write) / time; median (min..max) of %d samples" % REPS)
    for n in (128, 512, 2048, 4096):
        byts = 2.0 * sum(r * w(n) for r, w, _p in shapes.values())
        res = {"kernel": [], "runtime": []}
        for rep in range(REPS):
            for side in ("kernel", "runtime") if rep % 2 == 0 else ("runtime", "kernel"):
                res[side].append(kernel_ms(n) if side == "kernel" else runtime_ms(n))
        (km, klo, khi), (rm, rlo, rhi) = med(res["kernel"]), med(res["runtime"])
        print("n=%5d  %7.1f MB  kv_copy kernel %.4f ms (%.4f..%.4f) %7.1f GB/s   hipMemcpy2DAsync x2 %.4f ms (%.4f..%.4f) %7.1f GB/s   kernel/runtime %.3f"
              % (n, byts / 2e6, km, klo, khi, byts / km / 1e6, rm, rlo, rhi, byts / rm / 1e6, km / rm), flush=True)


def ttft():
    name = "mistral-7b"
    cfg = MODEL_CONFIGS[name]
    wts = bench.synth_device_weights(torch, cfg, torch.device("cuda", 0))
    gm = fa.Model(cfg, bench.as_fl_tensors(wts, 0), dtype="bf16")
    del wts
    torch.cuda.empty_cache()
    rs = np.random.RandomState(0)
    print("# time to first token, %s bf16 synthetic: (a) whole prompt on a fresh cache, (b) copy_prefix + 32-token suffix; median (min..max) of %d samples of 3"
          % (name, REPS))
    for npre in (512, 2048):
        T = npre + 32
        p = rs.randint(0, cfg["vocab_size"], size=T).astype(np.uint32)
        src, c = gm.new_cache(T + 8), gm.new_cache(T + 8)
        gm.forward_argmax(src, p[:npre], 0)

        def full():
            c.reset()
            return gm.forward_argmax(c, p, 0)

        def reuse():
            c.copy_prefix(src, npre)
            return gm.forward_argmax(c, p[npre:], npre)

        toks = (full(), reuse())
        res = {"a": [], "b": []}
        for rep in range(REPS):
            for side in ("a", "b") if rep % 2 == 0 else ("b", "a"):
                f = full if side == "a" else reuse
                f()
                gm.synchronize()
                t0 = time.perf_counter()
                for _ in range(3):
                    f()
                gm.synchronize()
                res[side].append((time.perf_counter() - t0) / 3 * 1e3)
        (am, alo, ahi), (bm, blo, bhi) = med(res["a"]), med(res["b"])
        print("prompt %4d + 32: (a) %.3f ms (%.3f..%.3f)   (b) %.3f ms (%.3f..%.3f)   b/a %.3f   first token a/b %d/%d"
              % (npre, am, alo, ahi, bm, blo, bhi, bm / am, toks[0], toks[1]), flush=True)
        src.close()
        c.close()


if "copy" in what:
    copy_rate()
if "ttft" in what:
    ttft()
