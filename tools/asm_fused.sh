#!/bin/bash
# Device assembly of the library ($OUT/ellc.s), the fused Gauss-Newton kernels cut out of it, their register / scratch use
# and the instruction count of the tolerance-mode pixel loop (one step = one pixel). usage: tools/asm_fused.sh [outdir]
set -e
OUT=${1:-/tmp/asm}
TOOLS=$(cd "$(dirname "$0")" && pwd)
mkdir -p $OUT
cd "$(dirname "$0")/../egomotion_with_local_loop_closures_amd/csrc"
/opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -w -S --cuda-device-only -mllvm -amdgpu-kernarg-preload-count=16 -o $OUT/ellc.s ellc_hip.hip
cut_kernel() { awk -v n="$1" 'index($0, n ":") == 1 {f = 1} f {print} /^\.Lfunc_end/ {if (f) exit}' $OUT/ellc.s > "$2"; }
cut_kernel _ZN4ellc12gn_fca_fusedILb0ELb1ELb1ELi0EEEvPKNS_10AlignStateEPKfiiiNS_9FusedArgsE $OUT/fused_fast.s
cut_kernel _ZN4ellc12gn_fca_fusedILb1ELb1ELb0ELin1EEEvPKNS_10AlignStateEPKfiiiNS_9FusedArgsE $OUT/fused_exact.s
# registers, scratch and occupancy of every Gauss-Newton kernel
awk '/^_ZN4ellc[0-9]+gn_[a-z_]+I.*:/ {name = $1} /^; NumVgprs:/ {if (name) v = $3} /^; ScratchSize:/ {if (name) s = $3}
     /^; Occupancy:/ {if (name) {print name, "vgpr", v, "scratch", s, "occupancy", $3; name = ""}}' $OUT/ellc.s
# tolerance mode: instructions of one pixel step on the interior path = the pixel loop's body (two steps, unrolled) without the basic
# blocks of the border paths, halved; with the weighted issue cost of tools/isa_cost.py. The border paths are priced beside it: what
# a wave with a lane on the border executes for its taps on top of the rest of the step (the packed path shares the interior's load)
python3 - $OUT/fused_fast.s "$TOOLS" <<'PY'
import re, sys
sys.path.insert(0, sys.argv[2])
import isa_cost
lines = open(sys.argv[1]).read().splitlines()
L = max(i for i, l in enumerate(lines) if "Inner Loop Header" in l)
label = lines[L].split(":")[0]
# the loop's basic blocks, wherever the layout put them: the header and every block marked "in Loop: Header=<it>"
allb, cur = [], []
for l in lines:
    if (l.startswith(".LBB") or l.startswith("; %bb.")) and cur:
        allb.append(cur); cur = []
    cur.append(l)
allb.append(cur)
mark = "Header=" + label[2:] + " "   # ".LBB48_62" is written "BB48_62" there
blocks = [b for b in allb if b[0].startswith(label + ":") or mark in b[0]]
def runs_of(anchors):
    # a path of each of the two steps is a contiguous run of blocks: from a step's first anchored block to its last
    out = set()
    if anchors:
        runs, start, prev = [], anchors[0], anchors[0]
        for i in anchors[1:]:
            if i - prev > 6: runs.append((start, prev)); start = i
            prev = i
        runs.append((start, prev))
        for a, b in runs: out.update(range(a, b + 1))
    return out
def has(b, *names): return any(n in l for l in b for n in names)
# the per-tap gathers (through r08 the border path; since r09 that of the diagnostic library's row loads only: none in this build)
gather = runs_of([i for i, b in enumerate(blocks) if has(b, "global_load_ubyte", "v_cmp_o_f32")])
# r09, the packed border path: the selectors and the combine (v_perm_b32, v_alignbyte_b32), and on the request side the block that
# clamps the window's origin in front of the one load both paths share (v_min_[iu]32 + v_cndmask_b32, no load, no branch)
packed = runs_of([i for i, b in enumerate(blocks) if has(b, "v_perm_b32", "v_alignbyte_b32")]) - gather
packed |= {i for i, b in enumerate(blocks) if has(b, "v_min_u32", "v_min_i32") and has(b, "v_cndmask_b32") and not has(b, "global_load", "s_cbranch", "v_rcp")} - gather
drop = gather | packed
def priced(idx):
    tot, cyc, slow = isa_cost.cost([l for i in sorted(idx) for l in blocks[i]])
    return tot, cyc
keep = [l for i, b in enumerate(blocks) if i not in drop for l in b]
tot, cyc, slow = isa_cost.cost(keep)
n = tot["fast"] + tot["slow"] + tot["trans"] + tot["cnd32"]
print("fast pixel step (interior path, per pixel): %.1f VALU instructions (fast class %.1f, slow %.1f, transcendental %.1f), %.1f others; modelled issue %.0f cycles per wave-step" %
      (n / 2, tot["fast"] / 2, (tot["slow"] + tot["cnd32"]) / 2, tot["trans"] / 2, tot["other"] / 2, cyc / 2))
for name, idx in (("packed border path (r09: the window at the clamped origin)", packed), ("per-tap gathers", gather)):
    if not idx: continue
    t, c = priced(idx)
    n = t["fast"] + t["slow"] + t["trans"] + t["cnd32"]
    loads = sum(1 for i in idx for l in blocks[i] if "global_load" in l or "buffer_load" in l)
    waits = sum(1 for i in idx for l in blocks[i] if "s_waitcnt vmcnt" in l)
    print("%s, the taps alone, per pixel: %.1f VALU instructions, %.1f others; modelled issue %.0f cycles per wave-step; %.1f vector loads and %.1f s_waitcnt vmcnt of its own" %
          (name, n / 2, t["other"] / 2, c / 2, loads / 2, waits / 2))
PY
