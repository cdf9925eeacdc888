"""Speculative greedy decode without a GPU: the six new entry points are exported and declared, fl_lookup / fl_spec_stats have the
header's sizes, fl_lookup_draft (a pure host function) equals a Python restatement of its rule, and the argument errors of
fl_forward_verify / fl_decode_lookup / fl_cache_truncate come back as FL_ERR_BAD_ARGUMENT with a message.

The restatement (lookup_draft_ref) and the seeded case list (draft_cases) are imported by tests/test_host_lookup.py, which runs the
same cases through the C++ header under the sanitizers."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fastllm_mi355x.h")
NEW = ("fl_cache_truncate", "fl_forward_verify", "fl_lookup_draft", "fl_decode_lookup", "fl_op_verify_select")


# ---- the rule, restated -------------------------------------------------------------------------------------------------------
def lookup_draft_ref(history, max_draft, ngram_max, ngram_min, limit):
    h = [int(x) for x in history]
    want = min(max_draft, limit)
    if want <= 0:
        return []
    for n in range(ngram_max, ngram_min - 1, -1):
        if n >= len(h):
            continue
        pat = h[len(h) - n:]
        for s in range(len(h) - n - 1, -1, -1):          # the largest s with s + n < len(h)
            if h[s:s + n] == pat:
                return h[s + n:s + n + want]             # (cut to the end of history by the slice)
    return []


def draft_cases():
    """[(history, max_draft, ngram_max, ngram_min, limit)]: 2 000 seeded random ones and the named edge cases."""
    rs = np.random.RandomState(1234)
    out = []
    for i in range(2000):
        alpha = (2, 4, 50)[i % 3]
        n = int(rs.randint(0, 201))
        h = rs.randint(0, alpha, size=n).tolist()
        nmax = int(rs.randint(1, 9))
        nmin = int(rs.randint(1, nmax + 1))
        out.append((h, int(rs.randint(0, 16)), nmax, nmin, int(rs.randint(0, 20))))
    out += [
        ([1, 2, 3, 4, 5, 6, 7], 7, 3, 1, 7),                                # no match
        ([9, 5, 1, 8, 5, 2, 7, 5], 4, 3, 1, 4),                             # match only at ngram_min (1): most recent 5 -> [2, 7, 5]
        ([9, 5, 1, 8, 5, 2, 7, 5], 4, 3, 2, 4),                             # ... and none when ngram_min is 2
        ([3, 3, 3, 3], 7, 3, 1, 7),                                         # the pattern overlaps its own earlier occurrence (aaaa)
        ([3, 3, 3, 3], 7, 2, 2, 7),
        ([1, 2, 7, 7, 1, 2, 8, 8, 1, 2], 2, 2, 2, 5),                       # two candidates: the most recent wins -> [8, 8]
        ([4, 6, 1, 4, 6], 7, 2, 1, 15),                                     # the continuation is shorter than max_draft -> [1, 4, 6]
        ([4, 6, 1, 4, 6], 7, 2, 1, 0),                                      # limit 0
        ([4, 6, 1, 4, 6], 7, 2, 1, 1),                                      # limit 1
        ([4, 6, 1, 4, 6], 0, 2, 1, 5),                                      # max_draft 0
        ([5, 5], 7, 2, 2, 7),                                               # n_history <= n: nothing to search with
        ([5, 5], 7, 8, 1, 7),                                               # ... but n = 1 still finds [5]
        ([5], 7, 1, 1, 7),
        ([], 7, 3, 1, 7),
    ]
    return out


def test_restatement_on_the_named_cases():
    r = lookup_draft_ref
    assert r([1, 2, 3, 4, 5, 6, 7], 7, 3, 1, 7) == []
    assert r([9, 5, 1, 8, 5, 2, 7, 5], 4, 3, 1, 4) == [2, 7, 5]
    assert r([9, 5, 1, 8, 5, 2, 7, 5], 4, 3, 2, 4) == []
    assert r([3, 3, 3, 3], 7, 3, 1, 7) == [3]                               # s = 0: [3,3,3] then the one id after it
    assert r([3, 3, 3, 3], 7, 2, 2, 7) == [3]                               # s = 1 (most recent), one id after it
    assert r([1, 2, 7, 7, 1, 2, 8, 8, 1, 2], 2, 2, 2, 5) == [8, 8]
    assert r([4, 6, 1, 4, 6], 7, 2, 1, 15) == [1, 4, 6]
    assert r([4, 6, 1, 4, 6], 7, 2, 1, 0) == [] and r([4, 6, 1, 4, 6], 7, 2, 1, 1) == [1]
    assert r([5, 5], 7, 2, 2, 7) == [] and r([5, 5], 7, 8, 1, 7) == [5] and r([5], 7, 1, 1, 7) == []


# ---- the ABI surface ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    import fastllm_amd
    return fastllm_amd.lib()


def test_new_symbols_are_exported_and_declared(L):
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        assert hasattr(L, name), name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    out = subprocess.check_output(["nm", "-D", "--defined-only", __import__("fastllm_amd").binding.LIB_PATH], text=True)
    assert set(NEW) <= set(re.findall(r" T (fl_[a-z_0-9]+)", out))
    assert re.search(r"#define\s+FL_VERIFY_MAX_DRAFT\s+15\b", hdr)
    assert L.fl_abi_version() == 2                                           # the change only adds entries


def test_struct_sizes_match_the_header():
    import fastllm_amd.binding as B
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(src, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) { printf("%%zu %%zu %%zu %%zu\\n", sizeof(fl_lookup), '
                             'sizeof(fl_spec_stats), offsetof(fl_lookup, ngram_min), offsetof(fl_lookup, _reserved)); return 0; }\n' % HEADER)
        subprocess.run(["gcc", "-std=c11", src, "-o", exe], check=True)
        sl, ss, o_min, o_res = (int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split())
    assert sl == C.sizeof(B.FlLookup) == 40 and ss == C.sizeof(B.FlSpecStats) == 24
    assert o_min == B.FlLookup.ngram_min.offset == 12 and o_res == B.FlLookup._reserved.offset == 24
    assert B.VERIFY_MAX_DRAFT == 15


def test_lookup_draft_equals_the_restatement():
    import fastllm_amd as fa
    cases = draft_cases()
    assert len(cases) >= 2000
    n_hit = 0
    for h, md, nmax, nmin, limit in cases:
        got = fa.lookup_draft(h, limit, max_draft=md, ngram_max=nmax, ngram_min=nmin).tolist()
        want = lookup_draft_ref(h, md, nmax, nmin, limit)
        assert got == want, (h, md, nmax, nmin, limit, got, want)
        n_hit += bool(want)
    assert 200 < n_hit < len(cases)                                          # the random cases cover both outcomes


def test_lookup_draft_argument_errors(L):
    import fastllm_amd.binding as B
    h = np.array([1, 2, 1, 2], np.uint32)
    out = np.zeros(8, np.uint32)
    n = C.c_size_t(99)

    def rc(o, hist=h.ctypes.data, outp=out.ctypes.data, np_=C.byref(n)):
        return L.fl_lookup_draft(hist, h.size, C.byref(o) if o is not None else None, 8, outp, np_)

    assert rc(B.make_lookup()) == 0 and n.value == 2 and out[:2].tolist() == [1, 2]
    o = B.make_lookup()
    o.struct_size -= 8
    assert rc(o) == -8 and b"struct_size" in L.fl_last_error()
    assert rc(B.make_lookup(ngram_max=2, ngram_min=3)) == -8 and b"ngram_min" in L.fl_last_error()
    assert rc(B.make_lookup(ngram_max=9)) == -8 and rc(B.make_lookup(ngram_min=0)) == -8
    assert rc(B.make_lookup(max_draft=16)) == -8 and b"max_draft" in L.fl_last_error()
    assert rc(B.make_lookup(max_draft=-1)) == -8
    assert rc(None) == -8 and b"null" in L.fl_last_error()
    assert rc(B.make_lookup(), hist=None) == -8 and rc(B.make_lookup(), outp=None) == -8 and rc(B.make_lookup(), np_=None) == -8
    assert n.value == 0                                                      # a failed call leaves no stale count


def test_verify_and_loop_argument_errors(L):
    """No model can exist here without a GPU, so the handles are NULL: everything that is decided BEFORE the handles are looked at
    must say what is wrong (not "null model"), and a call whose only fault is the missing model says that."""
    import fastllm_amd.binding as B
    toks = np.zeros(17, np.uint32)
    dr = np.zeros(16, np.uint32)
    n = C.c_size_t(5)
    st = B.FlSpecStats()
    # fl_forward_verify
    assert L.fl_forward_verify(None, None, 1, dr.ctypes.data, 16, 0, toks.ctypes.data, C.byref(n), None) == -8
    assert b"FL_VERIFY_MAX_DRAFT" in L.fl_last_error()
    assert L.fl_forward_verify(None, None, 1, dr.ctypes.data, 3, 0, None, C.byref(n), None) == -8 and b"tokens_out" in L.fl_last_error()
    assert L.fl_forward_verify(None, None, 1, dr.ctypes.data, 3, 0, toks.ctypes.data, None, None) == -8 and b"n_out" in L.fl_last_error()
    assert L.fl_forward_verify(None, None, 1, None, 3, 0, toks.ctypes.data, C.byref(n), None) == -8 and b"draft" in L.fl_last_error()
    assert L.fl_forward_verify(None, None, 1, dr.ctypes.data, 15, 0, toks.ctypes.data, C.byref(n), None) == -8
    assert b"null model or cache" in L.fl_last_error() and n.value == 0
    # fl_decode_lookup
    o = B.make_lookup()

    def loop(opts, tokens=toks.ctypes.data, n_out=C.byref(n), steps=4):
        return L.fl_decode_lookup(None, None, dr.ctypes.data, 4, 1, 0, steps, -1, C.byref(opts) if opts is not None else None, tokens, n_out, C.byref(st))

    bad = B.make_lookup()
    bad.struct_size = 24
    assert loop(bad) == -8 and b"struct_size" in L.fl_last_error()
    assert loop(B.make_lookup(ngram_max=1, ngram_min=2)) == -8 and b"ngram_min" in L.fl_last_error()
    assert loop(B.make_lookup(max_draft=16)) == -8 and b"max_draft" in L.fl_last_error()
    assert loop(None) == -8
    assert loop(o, tokens=None) == -8 and b"tokens_out" in L.fl_last_error()
    assert loop(o, n_out=None) == -8 and b"n_out" in L.fl_last_error()
    assert loop(o) == -8 and b"null model or cache" in L.fl_last_error()
    assert loop(o, steps=0) == 0 and n.value == 0                            # nothing to do: fl_decode_greedy's answer
    # fl_cache_truncate
    assert L.fl_cache_truncate(None, 0) == -8 and b"null cache" in L.fl_last_error()
    # fl_op_verify_select: the shape checks come before the device probe; a well-formed call reaches the device or the loud "no device"
    lg = np.zeros((2, 8), np.float32)
    acc = C.c_int64(0)
    assert L.fl_op_verify_select(lg.ctypes.data, 17, 8, dr.ctypes.data, toks.ctypes.data, C.byref(acc)) == -8
    assert L.fl_op_verify_select(lg.ctypes.data, 0, 8, dr.ctypes.data, toks.ctypes.data, C.byref(acc)) == -8
    assert L.fl_op_verify_select(lg.ctypes.data, 2, 8, None, toks.ctypes.data, C.byref(acc)) == -8
    assert L.fl_op_verify_select(None, 2, 8, dr.ctypes.data, toks.ctypes.data, C.byref(acc)) == -8
    assert L.fl_op_verify_select(lg.ctypes.data, 2, 8, dr.ctypes.data, toks.ctypes.data, C.byref(acc)) in (0, -9)
