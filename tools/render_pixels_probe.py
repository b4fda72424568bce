#!/usr/bin/env python3
"""Developer probe: what rr_render_pixels costs next to rr_render and rr_shade_rays on the same frame.  The bench frame (sponza_syn
1280 x 720, 16 spp by default) on one handle with kernel_timing, the median of 7 calls of each of three routes: rr_render with the aux
buffers, rr_render_pixels without a list and with rgba8_out, and rr_shade_rays on the frame's primary rays (numpy's, pinhole).  Prints
host wall time (median, min, max), the device time and the three ms_* sums of the median call.  The whole-frame form runs rr_render's
launches plus a resolve of 36 B per pixel and its copy, so it should cost what rr_render costs; rr_shade_rays pays 40 B of records per
ray on level 1 and runs without sample groups.

usage: render_pixels_probe.py [scene [width height spp]] [--routes render,pixels,pixels_c,rays]"""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from rustray_amd import capi
from tools.shade_rays_probe import pinhole_rays

CALLS = 7


def main():
    argv = list(sys.argv[1:])
    routes = ("render", "pixels", "pixels_c", "rays")
    if "--routes" in argv:
        i = argv.index("--routes")
        routes = tuple(argv[i + 1].split(","))
        del argv[i:i + 2]
    scene = argv[0] if argv else "sponza_syn"
    w, h, spp = (int(a) for a in argv[1:4]) if len(argv) > 3 else (1280, 720, 16)
    fs, cam, cfg = bench.build_workload(scene, w, h, spp, 1)
    camc = cam.c_struct()
    table, cell = capi.sample_table(spp)
    calls = {}
    with capi.DeviceScene(fs, 0) as ds:
        ds.set_profiling(True)
        calls["render"] = lambda: ds.render(camc, cfg, aux=True)
        calls["pixels"] = lambda: ds.render_pixels(camc, cfg, None, rgba8=True)
        # the C call alone, into arrays that exist and have been touched: what the binding's column copies and fresh arrays add to "pixels"
        rec, byt = np.ones((w * h, 8), np.float32), np.ones((w * h, 4), np.uint8)
        calls["pixels_c"] = lambda: capi._check(capi.lib().rr_render_pixels(ds._h, C.byref(camc), C.byref(cfg), None, None, w * h, rec.ctypes.data, byt.ctypes.data, None))
        if "rays" in routes:
            o, d = pinhole_rays(camc, table, cell)
            calls["rays"] = lambda: ds.shade_rays(o, d, cfg, spp)
        print(f"{scene} {w}x{h}x{spp}: {w * h * spp} primary rays, median of {CALLS} calls (min .. max)")
        keep = {}
        for tag in routes:
            call = calls[tag]
            call()                                   # first use: buffers grow
            runs = []
            for _ in range(CALLS):
                t0 = time.perf_counter(); out = call(); wall = (time.perf_counter() - t0) * 1e3
                runs.append((wall, ds.stats()))
            keep[tag] = out
            runs.sort(key=lambda r: r[0])
            wall, st = runs[CALLS // 2]
            print(f"{tag:8s} host {wall:8.2f} ms ({runs[0][0]:8.2f} .. {runs[-1][0]:8.2f}, spread {runs[-1][0] - runs[0][0]:6.2f})  device {st['ms_total']:8.2f} ms  "
                  f"closest {st['ms_trace_closest']:7.2f}  shadow {st['ms_trace_shadow']:7.2f}  shade {st['ms_shade']:7.2f}  batches {st['batches']}  "
                  f"stages {ds.overlap_stages()}  rays p/s/sh {st['primary_rays']} / {st['secondary_rays']} / {st['shadow_rays']}")
    if "render" in keep and "pixels" in keep:
        f, p = keep["render"], keep["pixels"]
        same = np.array_equal(p["rgba"], f["rgba"].reshape(-1, 4)) and np.array_equal(p["depth"], f["depth"].reshape(-1)) and \
            np.array_equal(p["object_id"], f["object_id"].reshape(-1)) and np.array_equal(p["normal"], f["normal"].reshape(-1, 3), equal_nan=True)
        print(f"rr_render_pixels' bytes, depth, normal and id equal rr_render's: {same}")


if __name__ == "__main__":
    main()
