#!/usr/bin/env python3
"""Per kernel, are two `hipcc --cuda-device-only -S` outputs the same instruction stream?  (No GPU needed.)
    tools/isa_same.py parent.s new.s
Comments, directives and the numbers of local labels are dropped; prints `same` or `DIFF` with both lengths and, for a DIFF,
the opcodes whose counts moved (new - parent)."""
import collections
import re
import subprocess
import sys


def kernels(path):
    out, name = {}, None
    for line in open(path):
        line = line.split(";")[0].strip()
        m = re.match(r"^(_Z\w+):$", line)
        if m:
            name, out[name] = m.group(1), []
        elif line.startswith(".Lfunc_end"):
            name = None
        elif name and line and not line.startswith("."):
            out[name].append(re.sub(r"\.LBB\d+_\d+", ".LBB", line))
        elif name and re.match(r"^\.LBB\d+_\d+:$", line):
            out[name].append(".LBB:")
    return out


a, b = ({k: v for k, v in kernels(p).items() if "s_endpgm" in v} for p in sys.argv[1:3])
names = subprocess.run(["c++filt"], input="\n".join(sorted(set(a) | set(b))), capture_output=True, text=True).stdout.split("\n")
for sym, name in zip(sorted(set(a) | set(b)), names):
    x, y = a.get(sym), b.get(sym)
    name = name.split("(")[0].replace("void dm2::", "")
    if x is None or y is None:
        print(f"DIFF  {name}: only in {'new' if x is None else 'parent'}")
    elif x == y:
        print(f"same  {name}: {len(x)}")
    else:
        cx, cy = (collections.Counter(i.split()[0] for i in s if not i.endswith(":")) for s in (x, y))
        moved = " ".join(f"{op}{cy[op] - cx[op]:+d}" for op in sorted(set(cx) | set(cy)) if cx[op] != cy[op])
        print(f"DIFF  {name}: {len(x)} -> {len(y)}  {moved or '(order only)'}")
