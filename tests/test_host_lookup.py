"""The prompt-lookup search (fastllm_amd/csrc/lookup.h, the one copy api.hip also includes) as a stand-alone program under
AddressSanitizer + UndefinedBehaviorSanitizer: the seeded cases of tests/test_lookup_abi.py, read from a file, against the Python
restatement of the rule.  Every buffer the driver hands over is a heap block of exactly the promised size."""
import os
import subprocess

import pytest

from test_lookup_abi import draft_cases, lookup_draft_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lookup") / "test_host_lookup")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "fastllm_amd", "csrc"), os.path.join(ROOT, "tests", "host", "test_host_lookup.cc"), "-o", exe])
    return exe


def test_header_matches_the_restatement_under_sanitizers(driver, tmp_path):
    cases = draft_cases()
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        for h, md, nmax, nmin, limit in cases:
            f.write("%d %d %d %d %d %s\n" % (md, nmax, nmin, limit, len(h), " ".join(str(x) for x in h)))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([driver, str(path)], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0 and "host lookup driver done %d" % len(cases) in out.stdout, out.stdout[-2000:] + out.stderr[-6000:]
    rows = [[int(x) for x in ln.split()] for ln in out.stdout.splitlines() if ln and ln[0].isdigit()]
    assert len(rows) == len(cases)
    for (h, md, nmax, nmin, limit), row in zip(cases, rows):
        want = lookup_draft_ref(h, md, nmax, nmin, limit)
        assert row[0] == len(row) - 1 and row[1:] == want, (h, md, nmax, nmin, limit, row, want)
