#!/usr/bin/env python3
"""Developer probe: what the host loop of adaptive sampling costs next to the fused call.  One frame (sponza_syn 1280 x 720, monte_carlo,
16 -> 128 samples by default) on one handle, in one process.  The threshold is chosen once, from the base frame's half_error, so that
about a fifth of the frame is refined.  Two arms, wall time around the call, WARMUP frames each and then the median of FRAMES timed
frames with their spread:
  host loop  Raytracing.render_adaptive: rr_render_pixel_parts, half_error and refine_list in numpy, rr_render_pixels, a numpy scatter
  fused      Raytracing.render_adaptive_on_device: rr_render_adaptive
Then, with kernel_timing, the device time of the three launches that make the list (rr_frame_stats::ms_binning after a fused call), their
share of the fused call's device time and the bandwidth they achieved over the 64 B read and 4 + 4 B written per pixel and list entry.

usage: adaptive_time.py [scene [width height base_samples max_samples]] [--limit SECONDS]"""
import os
import signal
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from rustray_amd import adaptive
from rustray_amd.renderer import Raytracing

WARMUP, FRAMES, FRACTION = 3, 9, 0.2


def main():
    argv = list(sys.argv[1:])
    limit = 300
    if "--limit" in argv:
        i = argv.index("--limit")
        limit = int(argv[i + 1])
        del argv[i:i + 2]
    signal.alarm(limit)      # the probe's own time limit: SIGALRM ends the process
    scene = argv[0] if argv else "sponza_syn"
    w, h, base, top = (int(a) for a in argv[1:5]) if len(argv) > 4 else (1280, 720, 16, 128)
    fs, camera, cfg = bench.build_workload(scene, w, h, base, 1)
    rt = Raytracing(fs, camera, 0)
    try:
        rt.config = cfg
        ds = rt.device_scene
        first = ds.render_pixel_parts(camera.c_struct(), cfg, None, n_parts=2)
        err = adaptive.half_error(first["parts"]["color"])
        threshold = float(np.quantile(err, 1.0 - FRACTION))
        arms = {"host loop": lambda: rt.render_adaptive(base, top, threshold), "fused": lambda: rt.render_adaptive_on_device(base, top, threshold)}
        keep, median = {}, {}
        print(f"{scene} {w}x{h}, {base} -> {top} samples, threshold {threshold:.6g} (the {1.0 - FRACTION:.2f} quantile of the base frame's half_error)")
        for tag, call in arms.items():
            for _ in range(WARMUP):
                keep[tag] = call()
            runs = []
            for _ in range(FRAMES):
                t0 = time.perf_counter(); call(); runs.append((time.perf_counter() - t0) * 1e3)
            runs.sort()
            median[tag] = runs[FRAMES // 2]
            print(f"{tag:10s} wall {median[tag]:8.3f} ms median of {FRAMES} ({runs[0]:8.3f} .. {runs[-1]:8.3f}, spread {runs[-1] - runs[0]:6.3f}), {WARMUP} warm-up frames")
        a, b = keep["host loop"], keep["fused"]
        same = all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint32), np.ascontiguousarray(b[k]).view(np.uint32)) for k in ("color", "depth", "normal", "object_id", "samples", "error"))
        n, count = w * h, int(b["n_refined"])
        print(f"refined {count} of {n} pixels ({count / n:.3f}); the two arms agree bit for bit: {same}")
        print(f"host loop / fused = {median['host loop'] / median['fused']:.3f}")
        ds.set_profiling(True)
        lists, totals = [], []
        for _ in range(WARMUP + FRAMES):
            rt.render_adaptive_on_device(base, top, threshold)
            st = ds.stats()
            lists.append(st["ms_binning"]); totals.append(st["ms_total"])
        lists, totals = sorted(lists[WARMUP:]), sorted(totals[WARMUP:])
        ms_list, ms_total = lists[FRAMES // 2], totals[FRAMES // 2]
        moved = 64 * n + 4 * n + 4 * ((count + 63) // 64 * 64)
        print(f"list kernels (masks, scan, scatter; kernel_timing) {ms_list * 1e3:8.1f} us median ({lists[0] * 1e3:.1f} .. {lists[-1] * 1e3:.1f}), "
              f"{ms_list / (ms_total + ms_list):.4f} of the fused call's device time ({ms_total:.3f} ms in its two passes + the list); {moved / 1e6:.2f} MB moved: "
              f"{moved / (ms_list * 1e-3) / 1e9:.0f} GB/s")
    finally:
        rt.device_scene.close()


if __name__ == "__main__":
    main()
