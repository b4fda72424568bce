#!/usr/bin/env python3
"""Developer tool: STATIC vector-instruction count per source line of one kernel (hipcc -S -gline-tables-only, .loc directives).
Straight-line shading code executes once per hit, so for k_shade the static count is close to the dynamic one per path.
usage: tools/static_cost.py [--insn P[,P...]] [--classes] [<mangled kernel prefix, default _Z7k_shadeILb1> [top N]]
--insn: count the instructions whose mnemonic starts with one of these prefixes instead of "v_" (lane moves: --insn v_readlane,v_writelane).
--classes: one row per kernel build matching the prefix: VALU, SALU, SMEM, VMEM (global_ / flat_ / buffer_ / scratch_), LDS and lane moves."""
import collections
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rustray_amd.capi import LIB_SOURCES  # noqa: E402

asm = os.path.join(ROOT, "build", "rr_api_g.s")
csrc = os.path.join(ROOT, "rustray_amd", "csrc")
os.makedirs(os.path.dirname(asm), exist_ok=True)
if not os.path.exists(asm) or os.path.getmtime(asm) < max(os.path.getmtime(os.path.join(csrc, f)) for f in LIB_SOURCES):
    subprocess.check_call(["hipcc", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize", "--offload-arch=gfx950", "-Wno-unused-function",
                           "-gline-tables-only", "-S", "--cuda-device-only", "-o", asm, "rr_api.hip"], cwd=csrc, stderr=subprocess.DEVNULL)
lines = open(asm).read().splitlines()
files = {}
for l in lines:
    m = re.match(r'\s*\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', l)
    if m:
        files[int(m.group(1))] = (m.group(3) or m.group(2)).split("/")[-1]
TOOLCHAIN = "<toolchain headers>"
argv = sys.argv[1:]
insn, classes = ("v_",), False
while argv and argv[0].startswith("--"):
    if argv[0] == "--insn": insn = tuple(argv[1].split(",")); argv = argv[2:]
    elif argv[0] == "--classes": classes = True; argv = argv[1:]
    else: sys.exit(__doc__)
prefix = argv[0] if len(argv) > 0 else "_Z7k_shadeILb1"
top = int(argv[1]) if len(argv) > 1 else 50

def mnemonics(body):
    for l in body:
        t = l.strip()
        if l.startswith("\t") and t and not t.startswith((".", ";")): yield t.split()[0]

if classes:
    CLASSES = (("valu", ("v_",)), ("salu", ("s_",)), ("smem", ("s_load", "s_buffer_load")), ("vmem", ("global_", "flat_", "buffer_", "scratch_")), ("lds", ("ds_",)),
               ("lane_moves", ("v_readlane", "v_writelane")))
    for s0 in [i for i, l in enumerate(lines) if l.startswith(prefix) and ": ; @" in l]:
        e0 = [i for i, l in enumerate(lines) if i > s0 and l.startswith(".Lfunc_end")][0]
        ms = list(mnemonics(lines[s0:e0]))
        row = {n: sum(m.startswith(p) for m in ms) for n, p in CLASSES}
        row["salu"] -= row["smem"]  # (scalar loads are counted on their own)
        name = subprocess.run(["c++filt", lines[s0].split(":")[0]], capture_output=True, text=True).stdout.split("(")[0].replace("void ", "").strip()
        name = re.sub(r"HIP_vector_type<float, 4u>", "float4", name)
        print(f"{name:44s} " + " ".join(f"{n} {c:5d}" for n, c in row.items()))
    sys.exit(0)
start = [i for i, l in enumerate(lines) if l.startswith(prefix)][0]
end = [i for i, l in enumerate(lines) if i > start and l.startswith(".Lfunc_end")][0]
cur, cnt = None, collections.Counter()
for l in lines[start:end]:
    m = re.match(r"\s*\.loc\s+(\d+)\s+(\d+)", l)
    if m:
        f = files.get(int(m.group(1)), "?")
        cur = (f, int(m.group(2))) if f in LIB_SOURCES else (TOOLCHAIN, 0)  # (the compiler's own headers: __ballot, __shfl, ...)
        continue
    t = l.strip()
    if l.startswith("\t") and t and not t.startswith((".", ";")) and t.split()[0].startswith(insn):
        cnt[cur] += 1
print(prefix, "static VALU instructions:" if insn == ("v_",) else "static " + ",".join(insn) + " instructions:", sum(cnt.values()))
byfile = collections.Counter()
for (f, _), c in cnt.items():
    byfile[f] += c
print(byfile.most_common(6))
src = {f: open(os.path.join(csrc, f)).read().splitlines() for f in LIB_SOURCES if f in byfile}
for f in src:
    items = sorted(((l, c) for (ff, l), c in cnt.items() if ff == f), key=lambda x: -x[1])[:top]
    for l, c in sorted(items):
        print(f"{f}:{l:5d} {c:5d}  {src[f][l - 1].strip()[:120]}")
