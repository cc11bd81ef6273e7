#!/usr/bin/env python3
"""Which kernels did a change of csrc/ touch?  python3 profiles/kernel_asm_diff.py parent.s this.s [--json out.json]
Both files are the device side of rt_api.hip (the Makefile's flags plus --cuda-device-only -S).  Each is split per kernel; comment
lines, directives and blank lines are dropped and the function number of local labels (.LBB<fn>_<block>) is masked, so that what
is compared is the instruction sequence.  Per kernel: identical or not, the instruction counts, and VGPRs, SGPRs, scratch bytes and
occupancy of both sides from the resource comments the assembler writes after each kernel.  Exit status 1 if a kernel exists on one side only."""
import json
import re
import subprocess
import sys


def demangle(names):
    out = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, out))


def kernels(path):
    lines = open(path).read().split("\n")
    names = [m.group(1) for l in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)] if m]
    res = {}
    for name in names:
        start = next(i for i, l in enumerate(lines) if l.split(";")[0].strip() == name + ":")
        end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith(".Lfunc_end"))
        body = []
        for l in lines[start + 1:end]:
            t = l.split(";")[0].strip()
            if not t or (t.startswith(".") and not t.startswith(".LBB")):
                continue
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", t))
        info = {}
        for l in lines[end:end + 80]:
            m = re.match(r"\s*;\s*(NumVgprs|TotalNumSgprs|ScratchSize|Occupancy):\s*(\d+)", l)
            if m and m.group(1) not in info:
                info[m.group(1)] = int(m.group(2))
        res[name] = (body, info)
    return res


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    dm = demangle(sorted(set(a) | set(b)))
    rows, lone = [], []
    for name in sorted(set(a) | set(b), key=lambda n: dm[n]):
        if name not in a or name not in b:
            lone.append(dm[name])
            continue
        (ba, ia), (bb, ib) = a[name], b[name]
        side = lambda i, body: dict(vgpr=i.get("NumVgprs"), sgpr=i.get("TotalNumSgprs"), scratch=i.get("ScratchSize"), occupancy=i.get("Occupancy"), instructions=len(body))
        rows.append(dict(kernel=dm[name], identical=ba == bb, parent=side(ia, ba), this=side(ib, bb)))
    diff = [r for r in rows if not r["identical"]]
    out = dict(kernels=len(rows), identical=len(rows) - len(diff), differing=[r["kernel"] for r in diff], on_one_side_only=lone, table=rows)
    for r in diff:
        print("differs: %s\n    parent %s\n    this   %s" % (r["kernel"], r["parent"], r["this"]))
    print("%d of %d kernels identical" % (out["identical"], out["kernels"]))
    if "--json" in sys.argv:
        json.dump(out, open(sys.argv[sys.argv.index("--json") + 1], "w"), indent=1)
    return 1 if lone else 0


if __name__ == "__main__":
    sys.exit(main())
