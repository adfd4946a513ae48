#!/usr/bin/env python3
"""Compare two device-only assembly files (hipcc --cuda-device-only -S) per
symbol: the instructions of every function, the .amdhsa_kernel descriptor and
the metadata entry (registers, LDS, scratch, arguments) of every kernel.
Prints the symbols only one file has and those that differ; exit status 1 if
there is any.
  python3 scripts/isa_diff.py before.s after.s"""
import re
import sys


def split(path):
    s = open(path).read()
    parts = {}
    for m in re.finditer(r"^(\w+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:", s, re.M | re.S):
        parts["text " + m.group(1)] = m.group(2)
    for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n(.*?)^\t\.end_amdhsa_kernel", s, re.M | re.S):
        parts["desc " + m.group(1)] = m.group(2)
    meta = s[s.find("amdhsa.kernels:"):]
    for blk in re.split(r"\n  - ", meta)[1:]:
        nm = re.search(r"\.name:\s+(\S+)", blk)
        if nm:
            parts["meta " + nm.group(1)] = blk.split("\namdhsa.")[0]
    return parts


a, b = split(sys.argv[1]), split(sys.argv[2])
only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
diff = sorted(k for k in set(a) & set(b) if a[k] != b[k])
for tag, names in (("only in " + sys.argv[1], only_a), ("only in " + sys.argv[2], only_b), ("differs", diff)):
    for n in names:
        print("%s: %s" % (tag, n))
print("%d symbols, %d identical" % (len(set(a) | set(b)), len(set(a) & set(b)) - len(diff)))
sys.exit(1 if only_a or only_b or diff else 0)
