"""CPU tests of top-p / top-k outside the kernel: the host mirror's LogitsProcessor (fastllm_amd/host/fastllm_host.hpp) against the
numpy restatement in topp_checker.py, as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer; and the argument
errors of the fl_*_ex entry points, which are decided before the device is looked for."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import topp_checker as tc
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "fastllm_amd", "lib")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("topp") / "test_host_top_p")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host", "test_host_top_p.cc"), "-o", exe,
                           "-L" + LIBDIR, "-lfastllm_mi355x", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def run(driver, tmp_path, prs, top_p, top_k, seed, skip, draws):
    path = tmp_path / "prs.f32"
    prs.astype(np.float32).tofile(path)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([driver, str(path), repr(float(top_p or 0.0)), str(int(top_k or 0)), str(seed), str(skip), str(draws)],
                         capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0 and "host top-p driver done" in out.stdout, out.stdout[-2000:] + out.stderr[-6000:]
    rows = [ln.split() for ln in out.stdout.splitlines() if ln and ln[0].isdigit()]
    return np.array([int(r[0]) for r in rows]), np.array([int(r[1]) for r in rows])


def cases():
    rs = np.random.RandomState(3)
    rnd = tc.prs_of((rs.randn(320) * 2.5).astype(np.float32), 0.8)
    ties = tc.prs_of((np.log(2.0) * rs.randint(-8, 1, size=2048)).astype(np.float32), 1.0)
    tail = tc.prs_of(np.concatenate([np.full(64, 5.0), np.full(2048 - 64, -12.0)]).astype(np.float32), 1.0)
    two = np.zeros(500, np.float32); two[[17, 432]] = 0.5
    return [("random p", rnd, 0.9, None), ("random k", rnd, None, 8), ("random p+k", rnd, 0.9, 5), ("random k>m", rnd, 0.5, 40),
            ("ties p", ties, 0.9, None), ("ties k", ties, None, 300), ("tail exact", tail, 0.5, None), ("tail", tail, 0.9999, None),
            ("off", rnd, 1.0, 320), ("k=1 ties", two, None, 1)]


@pytest.mark.parametrize("name,prs,top_p,top_k", cases(), ids=[c[0] for c in cases()])
def test_host_logits_processor_matches_checker(driver, tmp_path, name, prs, top_p, top_k):
    seed, skip, n = 5, 2, 200
    toks, kept = run(driver, tmp_path, prs, top_p, top_k, seed, skip, n)
    chk = tc.Checker(prs, top_p, top_k)
    assert len(toks) == n and (kept == chk.m).all(), (kept[:4], chk.m)
    # the host mirror does the checker's arithmetic in the checker's order on the same probabilities: no draw may differ
    assert tc.compare_draws(toks, chk, seed, draws_done=skip) == 0
    if name == "tail exact":
        assert chk.m == 32 and toks.max() < 32
    if name == "k=1 ties":
        assert (toks == 17).all()                     # the LOWEST maximal index (ArgMax would keep 432)
    if name == "off":
        assert chk.m == prs.size


def test_argument_errors_precede_the_device_probe():
    import fastllm_amd as fa
    b = fa.binding
    L = fa.lib()
    lg = np.zeros(16, np.float32)
    out = np.zeros(2, np.uint32)

    def rc(sp):
        return L.fl_op_sample_ex(lg.ctypes.data, lg.size, C.byref(sp), 2, out.ctypes.data, None)

    assert rc(b.make_sampler(0.8, top_p=float("nan"))) == -8 and b"NaN" in L.fl_last_error()
    assert rc(b.make_sampler(0.8, top_k=-1)) == -8 and b"top_k" in L.fl_last_error()
    sp = b.make_sampler(0.8, top_p=0.9)
    sp.struct_size -= 8
    assert rc(sp) == -8 and b"struct_size" in L.fl_last_error()
    assert C.sizeof(b.FlSampler) == 56
    # a well-formed sampler gets past the checks: to the device, or to the loud "no device"
    assert rc(b.make_sampler(0.8, top_p=0.9, top_k=4)) in (0, -9)
