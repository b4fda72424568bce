#!/usr/bin/env python3
"""Developer probe: the dispatch TIMELINE of one frame (every kernel launch with its start offset, duration and the idle gap before
it), from `rocprofv3 --kernel-trace`.  Shows what a frame pays besides kernel time: level read-backs, launch gaps, small launches.
usage (GPU box): python tools/timeline.py run <n_ranks_share> [scene spp]   -> renders rank 0's share of an n-way tiling 4 times
                 rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/timeline.py run 8 ; python tools/timeline.py show DIR"""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

if sys.argv[1] == "run":
    import torch
    import bench
    from rustray_amd import capi
    from rustray_amd.renderer import TiledFrame, render_region_torch
    n = int(sys.argv[2])
    scene = sys.argv[3] if len(sys.argv) > 3 else "sponza_syn"
    spp = int(sys.argv[4]) if len(sys.argv) > 4 else 128
    fs, cam, cfg = bench.build_workload(scene, 1280, 720, spp, 1)
    ds = capi.DeviceScene(fs, 0)
    camc = cam.c_struct()
    tf = TiledFrame(1280, 720, 0, n, 32, 8)
    for _ in range(4):
        render_region_torch(ds, camc, cfg, tf, aux=True)
        torch.cuda.synchronize()
    ds.close()
else:
    f = max(glob.glob(os.path.join(sys.argv[2], "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)
    rows = [r for r in csv.DictReader(open(f))]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    # the last frame = from its first k_trace_closest<true> launch (level 1 in stages has one per stage) to its k_resolve
    names = [r["Kernel_Name"] for r in rows]
    resolves = [i for i, nm in enumerate(names) if "k_resolve" in nm]
    last = resolves[-1]
    first = min(i for i in range(resolves[-2] + 1 if len(resolves) > 1 else 0, last) if "k_trace_closest<true>" in names[i])
    t0 = int(rows[first]["Start_Timestamp"])
    prev_end = t0
    busy = covered = 0
    print(f"{'kernel':44s} {'queue':>5s} {'start us':>9s} {'end us':>9s} {'dur us':>8s} {'gap us':>7s}")
    for r in rows[first:last + 1]:
        s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
        nm = r["Kernel_Name"].split("(")[0].replace("void ", "")
        # gap: the device idle before this launch (launches of the staged level 1 overlap: negative = it started beside another)
        print(f"{nm[:44]:44s} {r.get('Queue_Id', '?'):>5s} {(s - t0) / 1e3:9.1f} {(e - t0) / 1e3:9.1f} {(e - s) / 1e3:8.1f} {(s - prev_end) / 1e3:7.1f}")
        busy += e - s
        covered += max(0, e - max(s, prev_end))
        prev_end = max(prev_end, e)
    total = prev_end - t0
    print(f"frame (level-1 launch to resolve): {total / 1e3:.1f} us, sum of kernel durations {busy / 1e3:.1f} us, no kernel running {(total - covered) / 1e3:.1f} us, "
          f"{last - first + 1} dispatches")
