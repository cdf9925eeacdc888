"""fl_op_linear_w4 / fl_op_linear_w4_plan and the "rows_w4" switch without a GPU: declared in the header, exported, bound by ctypes and
mirrored in the Rust extern block with the header's argument count; the ABI version did not move; argument errors and refusals precede
the device probe."""
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
    for name, n_args in (("fl_op_linear_w4", 12), ("fl_op_linear_w4_plan", 5)):
        c = re.search(r"\bint %s\s*\(([^;]*?)\)\s*;" % name, hdr, re.S)
        r = re.search(r"pub fn %s\s*\((.*?)\)\s*->\s*c_int;" % name, rust, re.S)
        assert c and r, name
        assert c.group(1).count(",") + 1 == n_args == len(re.findall(r"\w+\s*:", r.group(1))) == len(getattr(fa.lib(), name).argtypes)
        assert " T %s\n" % name in exported
    assert fa.lib().fl_abi_version() == 2 and hasattr(fa, "op_linear_w4") and hasattr(fa, "op_linear_w4_plan")


def test_argument_errors_and_refusals_need_no_device():
    x, q, e = np.zeros((2, 64), np.uint16), np.zeros((4, 32), np.uint8), np.full((4, 2), 127, np.uint8)
    y, b = np.full((2, 4), 7.0, np.float32), np.ones(4, np.float32)
    p = lambda a: a.ctypes.data if a is not None else None

    def rc(x=x, q=q, e=e, bias=None, T=2, N=4, K=64, epi=0, y=y):
        return fa.lib().fl_op_linear_w4(p(x), p(q), p(e), p(bias), None, T, N, K, epi, 0, None, p(y))

    assert rc(x=None) == rc(q=None) == rc(e=None) == rc(y=None) == BAD_ARGUMENT and b"null" in fa.lib().fl_last_error()
    assert rc(N=0) == rc(epi=2) == rc(epi=1, N=3) == rc(epi=1, bias=b) == BAD_ARGUMENT
    assert rc(T=1) == rc(T=17) == rc(K=48) == UNSUPPORTED and b"2..16 rows" in fa.lib().fl_last_error()
    assert (y == 7.0).all()
    plan = fa.op_linear_w4_plan
    assert plan(1, 64, 64) == plan(17, 64, 64) == plan(2, 64, 48) == plan(2, 64, 64, epilogue=2) == 0
    assert plan(2, 64, 64) == 1 and plan(16, 4096, 14336) > 1                  # more x than LDS holds: K slices ...
    assert plan(16, 4096, 14336, bias=True) == plan(16, 28672, 14336, epilogue=1) == 0     # ... which bias and gate/up cannot take


def test_the_switch_is_a_tune_key():
    fa.tune("rows_w4", 0)
