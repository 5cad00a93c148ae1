#!/usr/bin/env python3
"""The listing check of a pure move: every kernel of a parent's ISA listing is in
exactly one of the new listings, with the same instructions and the same kernel descriptor.

usage: python scripts/isa_same.py parent.s new.s [new.s ...]   (listings of `make asm`)

A kernel's parts are its function text (`<sym>:` to `.Lfunc_end`) and its `.amdhsa_kernel <sym>` ...
`.end_amdhsa_kernel` block; the function ordinal in local labels (and in the
comments that name them) is normalised. Text is compared, no
instruction is looked for. Exit status 1 when a kernel is missing, duplicated, extra or different.
"""
import re
import sys
from pathlib import Path

ORDINAL = re.compile(r"(\.L(?:BB|JTI|func_begin|func_end|tmp)|\bBB)\d+")   # labels, and BB<n>_ in comments


def normal(text):
    return re.sub(r"[ \t]+;", " ;", ORDINAL.sub(r"\1", text))   # (a comment's column moves with the ordinal's width)


def kernels(path):
    """{symbol: [(function text, descriptor), ...]} of one listing."""
    text = Path(path).read_text()
    found = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n.*?^\s*\.end_amdhsa_kernel$", text, re.M | re.S):
        sym = m.group(1)
        f = re.search(rf"^{re.escape(sym)}:.*?^\.Lfunc_end\d+:$", text, re.M | re.S)
        found.setdefault(sym, []).append((normal(f.group(0)) if f else None, m.group(0)))
    return found


parent = kernels(sys.argv[1])
new = {}
for path in sys.argv[2:]:
    for sym, parts in kernels(path).items():
        new.setdefault(sym, []).extend((path, p) for p in parts)
bad = 0
for sym in sorted(set(parent) | set(new)):
    want, got = parent.get(sym, []), new.get(sym, [])
    what = ("extra" if not want else "missing" if not got else
            "duplicated" if len(want) != 1 or len(got) != 1 else
            "different" if want[0] != got[0][1] or None in want[0] else None)
    if what:
        bad += 1
        print(f"{what}: {sym}" + "".join(f" [{p}]" for p, _ in got))
print(f"{len(parent)} kernels in the parent, {len(new)} in {len(sys.argv) - 2} new listing(s), {bad} finding(s)")
sys.exit(1 if bad else 0)
