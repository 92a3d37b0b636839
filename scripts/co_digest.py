#!/usr/bin/env python3
"""Digest of every gfx950 kernel of a built HIP library: one JSON line a kernel with its mangled name,
the code-object metadata scripts/check_isa.py reads (VGPRs, SGPRs, spill counts, private and group
segment sizes, dynamic stack) and a sha256 of its disassembly, sorted by name.

    python scripts/co_digest.py [path/to/libpolarcub_hip.so] > a.txt
    python scripts/co_digest.py --compare a.txt b.txt

The disassembly (llvm-objdump -d --no-show-raw-insn) is normalised before hashing: the leading
addresses, the trailing // comments and the zero padding behind a kernel's last instruction ("...") go,
so a kernel's position in its code object does not matter.
Two libraries whose digests compare equal hold the same machine code for every kernel, whichever
translation units and source text it came from.  --compare prints the kernels that differ, are missing
or occur more than once, then a summary line; exit status 1 unless identical.
"""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_isa import LLVM, ROOT, code_objects, kernel_metadata  # noqa: E402

_SYMBOL = re.compile(r"^[0-9a-f]+ <([^>]+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", re.S | re.M)


def _normalised(body):
    lines = []
    for line in body.splitlines():
        line = re.sub(r"^\s*[0-9a-f]+:\s*", "", line.split("//")[0]).strip()
        if line and line != "...":  # "...": zero padding up to the next symbol's alignment
            lines.append(re.sub(r"\s+", " ", line))
    return "\n".join(lines)


def disasm_hashes(lib):
    """[(symbol, sha256 of its normalised disassembly)] over every gfx950 code object of lib."""
    out = []
    with tempfile.TemporaryDirectory() as d:
        for i, co in enumerate(code_objects(lib)):
            f = os.path.join(d, "co%d.o" % i)
            with open(f, "wb") as fh:
                fh.write(co)
            text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", f], check=True,
                                  capture_output=True, text=True).stdout
            for m in _SYMBOL.finditer(text):
                out.append((m.group(1), hashlib.sha256(_normalised(m.group(2)).encode()).hexdigest()))
    return out


def digest(lib):
    """One dict a kernel (kernel_metadata's fields plus "sha256"), sorted by name; a kernel built in two
    translation units appears twice."""
    hashes = {}
    for name, h in disasm_hashes(lib):
        hashes.setdefault(name, []).append(h)
    rows = []
    for k in kernel_metadata(lib):
        hs = hashes.get(k["name"], [])
        # the copies of a kernel built more than once, in code-object order on both sides
        k["sha256"] = hs.pop(0) if hs else None
        rows.append(k)
    return sorted(rows, key=lambda k: (k["name"], k["sha256"] or ""))


def compare(a, b):
    rows = [[json.loads(line) for line in open(p) if line.strip()] for p in (a, b)]
    by = [{}, {}]
    for side, rs in zip(by, rows):
        for k in rs:
            side.setdefault(k["name"], []).append(k)
    bad = 0
    for name in sorted(set(by[0]) | set(by[1])):
        x, y = by[0].get(name, []), by[1].get(name, [])
        if len(x) != 1 or len(y) != 1:
            print("%s: %d time(s) in %s, %d in %s" % (name, len(x), a, len(y), b))
            bad += 1
        elif x[0] != y[0]:
            print("%s differs: %s" % (name, ", ".join("%s %s -> %s" % (f, x[0].get(f), y[0].get(f))
                                                      for f in sorted(set(x[0]) | set(y[0]))
                                                      if x[0].get(f) != y[0].get(f))))
            bad += 1
    print("%d kernel(s) in %s, %d in %s: %s" % (len(rows[0]), a, len(rows[1]), b,
                                                 "identical" if not bad else "%d difference(s)" % bad))
    return 1 if bad else 0


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--compare" in sys.argv:
        return compare(*args)
    lib = args[0] if args else os.path.join(ROOT, "polarcub_amd", "lib", "libpolarcub_hip.so")
    for k in digest(lib):
        print(json.dumps(k, sort_keys=True))
    return 0


if __name__ == "__main__":
    sys.exit(main())
