"""compile_guide (fastllm_amd/host/guide_compile.hpp, the one copy fastllm_host.hpp also includes) as a stand-alone program under
AddressSanitizer + UndefinedBehaviorSanitizer: tests/host/test_host_guide.cc holds the toy vocabulary, the byte DFAs and the CSR
arrays written out by hand."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("guide") / "test_host_guide")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "fastllm_amd", "host"), os.path.join(ROOT, "tests", "host", "test_host_guide.cc"), "-o", exe])
    return exe


def test_compile_guide_under_sanitizers(driver):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([driver], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0 and "host guide driver done 0" in out.stdout, out.stdout[-2000:] + out.stderr[-6000:]
