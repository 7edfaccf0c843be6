#!/usr/bin/env python3
"""Code object of two builds, kernel by kernel: registers, scratch, LDS, occupancy (which must be equal) and the instruction
stream (identical, or the two instruction counts). Input: two ellc.s as tools/asm_fused.sh writes them.
usage: tools/asm_compare.py PARENT/ellc.s NEW/ellc.s      exit status 1 when a resource figure differs"""
import re, shutil, subprocess, sys

FIELDS = ("NumVgprs", "NumAgprs", "ScratchSize", "LDSByteSize", "Occupancy")


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        if name is None:
            m = re.match(r"^(_Z\w+):", line)
            if m: name, body, res = m.group(1), [], {}
            continue
        m = re.match(r"^; (\w+): (\d+)", line)
        if m and m.group(1) in FIELDS: res[m.group(1)] = int(m.group(2))
        if m and m.group(1) == "Occupancy":
            out[name] = (res, body); name = None
            continue
        s = line.split(";")[0].strip()
        # (a local label carries the index of its function in the module, which moves when a kernel is added in front: .LBB12_3 -> .LBB_3)
        if s and not s.startswith(".") and not s.endswith(":"): body.append(re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s+", " ", s)))
    return out


def demangle(n):
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not filt: return n
    return subprocess.run([filt, n], capture_output=True, text=True).stdout.strip().split("(")[0].replace("void ellc::", "")


a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
bad = sorted(set(a) ^ set(b))
same = 0
print("| kernel | VGPR | scratch | LDS | occupancy | instructions parent -> new |\n|---|---|---|---|---|---|")
for n in a:
    if n not in b: continue
    (ra, ia), (rb, ib) = a[n], b[n]
    if ra != rb: bad.append(n)
    if ia == ib and ra == rb:
        same += 1
        continue
    print("| `%s` | %s | %s | %s | %s | %d -> %d |" % (demangle(n), *("%d" % ra[f] if ra[f] == rb[f] else "**%d -> %d**" % (ra[f], rb[f]) for f in ("NumVgprs", "ScratchSize", "LDSByteSize", "Occupancy")), len(ia), len(ib)))
print("%d kernels, %d with identical resources and instruction stream; %d differ in a resource figure or exist on one side only" % (len(a), same, len(bad)))
sys.exit(1 if bad else 0)
