#!/usr/bin/env python3
"""Do the kernels of one symbol family come out of the compiler unchanged?  Disassembles the gfx950 code objects of two builds of the
library and compares, symbol by symbol, every function whose (mangled) name contains PATTERN; branch targets and addresses are
normalised away (code that moved is not code that changed).  Runs without a GPU.

    python tools/kernel_disasm_diff.py OLD.so NEW.so [PATTERN]        (PATTERN defaults to gemv_kernel)
Exit status 0: same set of symbols, same instructions."""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
from test_dot_hazard import OBJDUMP, gfx950_code_objects  # noqa: E402


def functions(lib, pattern):
    out = {}
    for n, co in enumerate(gfx950_code_objects(open(lib, "rb").read())):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            dis = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", f.name], capture_output=True, text=True, check=True).stdout
        name = None
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.+)>:", line)
            if m:
                name = m.group(1) if pattern in m.group(1) and not m.group(1).startswith("L") else None
                if name:
                    out[name] = []
                continue
            if name and line.strip():
                text = line.split("//")[0].strip()
                if re.match(r"^s_(c?branch|call)", text):
                    text = text.split()[0] + " <target>"          # (an encoded distance: the same whenever the body between is)
                out[name].append(text)
    return out


def main():
    old, new = sys.argv[1], sys.argv[2]
    pattern = sys.argv[3] if len(sys.argv) > 3 else "gemv_kernel"
    a, b = functions(old, pattern), functions(new, pattern)
    bad = sorted(set(a) ^ set(b))
    for k in bad:
        print("only in %s: %s" % ("old" if k in a else "new", k))
    for k in sorted(set(a) & set(b)):
        if a[k] != b[k]:
            bad.append(k)
            print("differs: %s (%d vs %d instructions)" % (k, len(a[k]), len(b[k])))
    print("%d symbols with '%s' compared, %d differ" % (len(set(a) | set(b)), pattern, len(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
