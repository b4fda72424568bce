#!/usr/bin/env python3
"""Developer probe for the level-1 schedule: one line for the library in use (RUSTRAY_HIP_LIB picks a tools/variant.sh build) --
device time of the frame, the level-1 shade and shadow launch times, the number of stages that ran on two streams and the frame
checksum.  Variants built with -DRR_L1_OVERLAP=0 -DRR_SHADE_GRID_WG=k -DRR_SHADOW_GRID_WG=k give each kernel ALONE at k resident
workgroups per CU (profiles/r05_level1_share_rates.txt); -DRR_L1_SHADE_WG / RR_L1_SHADOW_WG / RR_L1_BUFFERS / RR_L1_STAGE_RAYS
give the splits, buffer counts and stage sizes of the two-stream path (profiles/r05_dropped.txt).
usage (GPU box): python tools/level1_share_probe.py [scene spp [frames]]"""
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from rustray_amd import capi

scene = sys.argv[1] if len(sys.argv) > 1 else "sponza_syn"
spp = int(sys.argv[2]) if len(sys.argv) > 2 else 128
frames = int(sys.argv[3]) if len(sys.argv) > 3 else 6
fs, cam, cfg = bench.build_workload(scene, 1280, 720, spp, 1)
camc = cam.c_struct()
with capi.DeviceScene(fs, 0) as ds:
    for _ in range(2):
        out = ds.render(camc, cfg)
    ms = []
    for _ in range(frames):
        ds.render(camc, cfg)
        ms.append(ds.stats()["ms_total"])
    ds.set_tuning(kernel_timing=1)
    ds.render(camc, cfg)
    ds.render(camc, cfg)
    st = ds.stats()
    stages = ds.overlap_stages() if hasattr(capi.lib(), "rr_scene_overlap_stages") else 0
name = os.path.basename(os.environ.get("RUSTRAY_HIP_LIB", "shipped"))
print(f"{name:28s} {scene} {spp} spp: frame ms median {statistics.median(ms):7.3f} min {min(ms):7.3f} max {max(ms):7.3f} | timed frame {st['ms_total']:7.3f}"
      f" closest1 {st['ms_trace_closest_level1']:6.3f} shade1 {st['ms_shade_level1']:6.3f} ({st['launches_shade_level1']}) shadow1 {st['ms_trace_shadow_level1']:6.3f}"
      f" ({st['launches_trace_shadow_level1']}) | stages {stages} checksum {int(out['rgba'].astype(np.int64).sum())}", flush=True)
