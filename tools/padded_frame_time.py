#!/usr/bin/env python3
"""Developer tool: time the frame of a bench scene padded with invisible items (tests/packet_pad.py pad_inert), i.e. the same
picture over a larger top level.  The library is RUSTRAY_HIP_LIB when set (an A/B build), as in tools/ab.sh.
usage: tools/padded_frame_time.py [--scene sponza_syn] [--items 512] [--mode scattered] [--steps 5] [--warmup 1] [--width 1280 --height 720 --spp 128]
Prints one JSON line: ms per frame (each step timed on its own, median and spread), the frame checksum and the ray counts."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="sponza_syn")
    ap.add_argument("--items", type=int, default=512)
    ap.add_argument("--mode", default="scattered")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--spp", type=int, default=128)
    args = ap.parse_args()
    import bench
    from rustray_amd import capi
    from tests.packet_pad import pad_inert
    fs, cam, cfg = bench.build_workload(args.scene, args.width, args.height, args.spp)
    n0 = len(fs.items)
    padded = pad_inert(fs, max(args.items, n0), args.mode, seed=args.items)
    camc = cam.c_struct()
    with capi.DeviceScene(padded, 0) as ds:
        ds.set_profiling(True)
        for _ in range(args.warmup):
            ds.render(camc, cfg)
        ms, out, st = [], None, None
        for _ in range(args.steps):
            t0 = time.perf_counter()
            out = ds.render(camc, cfg)
            st = ds.stats()
            ms.append((time.perf_counter() - t0) * 1000.0)
    print(json.dumps({"scene": args.scene, "items": len(padded.items), "items_unpadded": n0, "mode": args.mode, "ms_per_frame": ms,
                      "median_ms": float(np.median(ms)), "spread_ms": float(max(ms) - min(ms)),
                      "kernel_ms": {k: st[k] for k in ("ms_trace_closest", "ms_trace_shadow", "ms_shade", "ms_total")},
                      "rays": {k: int(st[k]) for k in ("primary_rays", "secondary_rays", "shadow_rays", "shaded_hits")},
                      "frame_checksum": int(out["rgba"].astype(np.int64).sum()), "lib": os.environ.get("RUSTRAY_HIP_LIB", "")}))


if __name__ == "__main__":
    main()
