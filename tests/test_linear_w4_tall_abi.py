"""fl_op_linear_w4_tall / fl_op_linear_w4_tall_plan without a GPU: declared in the header, exported, bound by ctypes and mirrored in
the Rust extern block with the header's argument count; argument errors and refusals precede the device probe; the 17-64-row and the
2-16-row hooks still refuse 65 rows."""
import os
import re
import subprocess

import numpy as np

import fastllm_amd as fa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARGUMENT, UNSUPPORTED = -8, -10


def test_declared_exported_bound_and_mirrored():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fastllm_mi355x.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "rust", "fastllm-mi355x", "src", "ffi.rs")).read()
    rust = rust[rust.index('extern "C" {'):]
    exported = subprocess.check_output(["nm", "-D", "--defined-only", fa.binding.LIB_PATH], text=True)
    for name, n_args in (("fl_op_linear_w4_tall", 11), ("fl_op_linear_w4_tall_plan", 4)):
        c = re.search(r"\bint %s\s*\(([^;]*?)\)\s*;" % name, hdr, re.S)
        r = re.search(r"pub fn %s\s*\((.*?)\)\s*->\s*c_int;" % name, rust, re.S)
        assert c and r, name
        assert c.group(1).count(",") + 1 == n_args == len(re.findall(r"\w+\s*:", r.group(1))) == len(getattr(fa.lib(), name).argtypes)
        assert " T %s\n" % name in exported
    assert fa.lib().fl_abi_version() == 2 and hasattr(fa, "op_linear_w4_tall") and hasattr(fa, "op_linear_w4_tall_plan")


def test_argument_errors_and_refusals_need_no_device():
    x, q, e = np.zeros((129, 64), np.uint16), np.zeros((4, 32), np.uint8), np.full((4, 2), 127, np.uint8)
    y = np.full((129, 4), 7.0, np.float32)
    p = lambda a: a.ctypes.data if a is not None else None

    def rc(x=x, q=q, e=e, T=65, N=4, K=64, epi=0, y=y):
        return fa.lib().fl_op_linear_w4_tall(p(x), p(q), p(e), None, T, N, K, epi, 0, None, p(y))

    assert rc(x=None) == rc(q=None) == rc(e=None) == rc(y=None) == BAD_ARGUMENT and b"null" in fa.lib().fl_last_error()
    assert rc(N=0) == rc(epi=2) == rc(epi=1, N=3) == BAD_ARGUMENT
    assert rc(T=64) == rc(T=129) == rc(K=48) == UNSUPPORTED and b"65..128 rows" in fa.lib().fl_last_error()
    assert (y == 7.0).all()
    plan = fa.op_linear_w4_tall_plan
    assert plan(64, 64, 64) == plan(129, 64, 64) == plan(65, 64, 48) == plan(65, 64, 64, epilogue=2) == 0
    assert plan(65, 64, 64) >= 1 and plan(128, 28672, 4096, epilogue=1) == 1
    assert fa.op_linear_w4_wide_plan(65, 64, 64) == fa.op_linear_w4_plan(65, 64, 64) == 0
