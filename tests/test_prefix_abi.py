"""K/V reuse across requests without a GPU: fl_cache_copy_prefix / fl_op_kv_copy are exported and declared and their argument errors
come back before the device is touched; PrefixIndex (fastllm_amd/host/fastllm_host.hpp, pure host code) through flh_prefix_index_*
against a Python restatement of its rule, on seeded random sequences and on the named cases."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_host_mirror import host  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fastllm_mi355x.h")
NEW = ("fl_cache_copy_prefix", "fl_op_kv_copy")
NEW_HOST = ("flh_prefix_index_create", "flh_prefix_index_match", "flh_prefix_index_insert", "flh_prefix_index_destroy",
            "flh_batcher_create_prefix", "flh_batcher_prefix_stats")


@pytest.fixture(scope="module")
def L():
    import fastllm_amd
    return fastllm_amd.lib()


def test_new_symbols_are_exported_and_declared(L, host):
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        assert hasattr(L, name), name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    out = subprocess.check_output(["nm", "-D", "--defined-only", __import__("fastllm_amd").binding.LIB_PATH], text=True)
    assert set(NEW) <= set(re.findall(r" T (fl_[a-z_0-9]+)", out))
    for name in NEW_HOST:
        assert hasattr(host, name), name
    assert re.search(r"#define\s+FL_ABI_VERSION\s+2\b", hdr) and L.fl_abi_version() == 2      # the change only adds entries


def test_copy_prefix_argument_errors(L):
    """No cache can exist here without a GPU, so the handles are NULL or stand-ins that are never dereferenced."""
    assert L.fl_cache_copy_prefix(None, None, 0) == -8 and b"null cache" in L.fl_last_error()
    assert L.fl_cache_copy_prefix(None, None, 5) == -8 and b"null cache" in L.fl_last_error()


def test_op_kv_copy_argument_errors(L):
    src = np.zeros((4, 64), np.uint8)
    dst = np.full((4, 128), 0xA5, np.uint8)
    ms = C.c_double(0)

    def rc(rows=4, width=32, sp=64, dp=128, s=src.ctypes.data, d=dst.ctypes.data):
        return L.fl_op_kv_copy(s, d, rows, width, sp, dp, 0, C.byref(ms))

    assert rc(s=None) == -8 and rc(d=None) == -8 and b"null" in L.fl_last_error()
    assert rc(width=31) == -8 and b"multiple of 2" in L.fl_last_error()                    # an odd width
    assert rc(width=0) == -8 and rc(width=-2) == -8 and rc(rows=0) == -8 and rc(rows=-1) == -8
    assert rc(sp=72) == -8 and b"multiples of 16" in L.fl_last_error()                     # a pitch that is no multiple of 16
    assert rc(dp=120) == -8
    assert rc(width=66) == -8 and b"at least the width" in L.fl_last_error()               # src pitch 64 < width
    assert rc(width=130, sp=256) == -8                                                     # dst pitch 128 < width
    assert (dst == 0xA5).all()                                                             # a refused call writes nothing
    assert rc() in (0, -9)                                                                 # well-formed: the device, or the loud "no device"


# ---- PrefixIndex, restated ------------------------------------------------------------------------------------------------------
class IndexRef:
    def __init__(self, entries):
        self.seqs, self.used, self.clock = [[] for _ in range(entries)], [0] * entries, 0

    @staticmethod
    def common(a, b):
        n = 0
        while n < min(len(a), len(b)) and a[n] == b[n]:
            n += 1
        return n

    def touch(self, e):
        self.clock += 1
        self.used[e] = self.clock

    def match(self, prompt, min_match):
        ns = [min(self.common(prompt, q), max(len(prompt) - 1, 0)) for q in self.seqs]
        n = max(ns)
        if n < max(min_match, 1):
            return -1, 0
        e = max((i for i in range(len(ns)) if ns[i] == n), key=lambda i: self.used[i])       # ties: the most recently used
        self.touch(e)
        return e, n

    def insert(self, ids):
        if not ids:
            return -1
        covered = [i for i, q in enumerate(self.seqs) if q[:len(ids)] == ids]               # ids is a prefix of a stored sequence
        if covered:
            self.touch(max(covered, key=lambda i: self.used[i]))
            return -1
        ext = [i for i, q in enumerate(self.seqs) if q and ids[:len(q)] == q]               # a stored sequence is a prefix of ids
        if ext:
            e = max(ext, key=lambda i: (len(self.seqs[i]), self.used[i]))
        else:
            e = min(range(len(self.seqs)), key=lambda i: (self.used[i], i))                 # least recently used, lowest index first
        self.seqs[e] = list(ids)
        self.touch(e)
        return e


class Index:
    def __init__(self, host, entries):
        host.flh_prefix_index_create.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
        host.flh_prefix_index_match.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_int64), C.POINTER(C.c_size_t)]
        host.flh_prefix_index_insert.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int64)]
        host.flh_prefix_index_destroy.argtypes = [C.c_void_p]
        host.flh_prefix_index_destroy.restype = None
        self.host, self.h = host, C.c_void_p()
        assert host.flh_prefix_index_create(entries, C.byref(self.h)) == 0, host.flh_last_error()

    def match(self, prompt, min_match):
        a = np.ascontiguousarray(prompt, dtype=np.uint32)
        e, n = C.c_int64(-7), C.c_size_t(99)
        assert self.host.flh_prefix_index_match(self.h, a.ctypes.data if a.size else None, a.size, min_match, C.byref(e), C.byref(n)) == 0
        return e.value, n.value

    def insert(self, ids):
        a = np.ascontiguousarray(ids, dtype=np.uint32)
        e = C.c_int64(-7)
        assert self.host.flh_prefix_index_insert(self.h, a.ctypes.data if a.size else None, a.size, C.byref(e)) == 0
        return e.value

    def close(self):
        self.host.flh_prefix_index_destroy(self.h)


@pytest.mark.parametrize("entries", [1, 2, 4])
def test_prefix_index_equals_the_restatement(host, entries):
    """4 000 seeded operations over a 4-letter alphabet (so that common prefixes, extensions and contained sequences all happen)."""
    rs = np.random.RandomState(77 + entries)
    idx, ref = Index(host, entries), IndexRef(entries)
    hits = stored = 0
    pool = []
    for step in range(4000):
        if pool and rs.rand() < 0.5:                           # a sequence related to an earlier one: cut or extended
            base = pool[int(rs.randint(len(pool)))]
            s = base[:int(rs.randint(0, len(base) + 1))] + rs.randint(0, 4, size=int(rs.randint(0, 6))).tolist()
        else:
            s = rs.randint(0, 4, size=int(rs.randint(0, 12))).tolist()
        pool = (pool + [s])[-16:]
        if rs.rand() < 0.5:
            mm = int(rs.randint(0, 6))
            got, want = idx.match(s, mm), ref.match(s, mm)
            hits += want[0] >= 0
        else:
            got, want = idx.insert(s), ref.insert(s)
            stored += want >= 0
        assert got == want, (step, s, got, want)
    assert hits > 200 and stored > 200
    idx.close()


def test_prefix_index_named_cases(host):
    idx = Index(host, 3)
    assert idx.match([1, 2, 3], 1) == (-1, 0)                                  # an empty index
    assert idx.insert([1, 2, 3, 4, 5, 6]) == 0
    # the cap at len - 1: a prompt that is stored whole still forwards its last token
    assert idx.match([1, 2, 3, 4, 5, 6], 1) == (0, 5)
    assert idx.match([1, 2, 3], 1) == (0, 2)
    assert idx.match([1], 1) == (-1, 0) and idx.match([], 0) == (-1, 0)
    # the min_match boundary: a common prefix of 4
    assert idx.match([1, 2, 3, 4, 9, 9], 4) == (0, 4)
    assert idx.match([1, 2, 3, 4, 9, 9], 5) == (-1, 0)
    assert idx.match([9, 2, 3], 0) == (-1, 0)                                  # nothing in common is a miss even at min_match 0
    # extend in place: the entry keeps its place
    assert idx.insert([1, 2, 3, 4, 5, 6, 7, 8]) == 0
    assert idx.match([1, 2, 3, 4, 5, 6, 7, 8, 9], 1) == (0, 8)
    # a prefix of a stored sequence (or the sequence itself) is not inserted
    assert idx.insert([1, 2, 3]) == -1 and idx.insert([1, 2, 3, 4, 5, 6, 7, 8]) == -1 and idx.insert([]) == -1
    idx.close()
    # LRU eviction order: never-used entries first (lowest index), then the least recently used
    idx = Index(host, 3)
    assert [idx.insert([10 * k, 1, 2]) for k in (1, 2, 3)] == [0, 1, 2]
    assert idx.match([10, 1, 2, 3], 1) == (0, 3)                               # entry 0 is now the most recent; 1 is the oldest
    assert idx.insert([40, 1, 2]) == 1
    assert idx.insert([50, 1, 2]) == 2
    assert idx.insert([60, 1, 2]) == 0
    assert idx.match([20, 1, 2, 3], 1) == (-1, 0) and idx.match([40, 1, 2, 3], 1) == (1, 3)
    idx.close()
    # a tie goes to the most recently used entry
    idx = Index(host, 3)
    assert idx.insert([7, 7, 7, 1]) == 0 and idx.insert([7, 7, 7, 2]) == 1
    assert idx.match([7, 7, 7, 3], 1) == (1, 3)                                # both share 3: entry 1 was used last
    assert idx.match([7, 7, 7, 1, 5], 1) == (0, 4)                             # (the longer match wins whatever the order)
    assert idx.match([7, 7, 7, 3], 1) == (0, 3)                                # ... and that made entry 0 the most recent
    idx.close()


def test_prefix_index_argument_errors(host):
    host.flh_prefix_index_create.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
    h = C.c_void_p()
    assert host.flh_prefix_index_create(0, C.byref(h)) == -8 and b"at least one entry" in host.flh_last_error()
    assert host.flh_prefix_index_create(2, None) == -8
