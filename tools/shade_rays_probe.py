#!/usr/bin/env python3
"""Developer probe: what rr_shade_rays costs next to rr_render on the same rays.  The bench frame (sponza_syn 1280 x 720, 16 spp by
default) with kernel_timing, once through rr_render and once through rr_shade_rays on that frame's primary rays (made here with
numpy, in float32; result y * w + x is the pixel).  Prints host wall time, the device time and the three ms_* sums per ray for both:
level 1 of the query reads and writes 40-B ray records that a frame derives from the ray's index, and runs the deeper levels' builds
of the kernels (no sample groups, no fixed shadow slots, no stages).

usage: shade_rays_probe.py [scene [width height spp]]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from rustray_amd import capi


def pinhole_rays(cam, table, cell):
    """primary_ray without depth of field, vectorised: (w * h * samples, 3) origins and un-normalised directions, pixel-major."""
    w, h = cam.width, cam.height
    f = np.float32
    pi = np.frombuffer(bytes(cam.projection_inverse), f).reshape(4, 4).T   # column-major -> math layout
    vi = np.frombuffer(bytes(cam.view_inverse), f).reshape(4, 4).T
    y, x, k = np.meshgrid(np.arange(h), np.arange(w), np.arange(len(table)), indexing="ij")
    xt = (f(2.0) / f(w)) * table[k, 0].astype(f) * (f(1.0) / f(cell))
    yt = (f(2.0) / f(h)) * table[k, 1].astype(f) * (f(1.0) / f(cell))
    sx = (((x.astype(f) + f(0.5)) / f(w)) * f(2.0) - f(1.0)) + xt
    sy = (f(1.0) - ((y.astype(f) + f(0.5)) / f(h)) * f(2.0)) + yt
    v = np.stack([sx, sy, np.full_like(sx, -1.0), np.ones_like(sx)], axis=-1).reshape(-1, 4)
    pp = v @ pi.T
    o = np.concatenate([pp[:, :3], np.ones((len(pp), 1), f)], axis=1) @ vi.T
    d = np.concatenate([pp[:, :3], np.zeros((len(pp), 1), f)], axis=1) @ vi.T
    return np.ascontiguousarray(o[:, :3], f), np.ascontiguousarray(d[:, :3], f)


def main():
    scene = sys.argv[1] if len(sys.argv) > 1 else "sponza_syn"
    w, h, spp = (int(a) for a in sys.argv[2:5]) if len(sys.argv) > 4 else (1280, 720, 16)
    fs, cam, cfg = bench.build_workload(scene, w, h, spp, 1)
    camc = cam.c_struct()
    table, cell = capi.sample_table(spp)
    o, d = pinhole_rays(camc, table, cell)
    n_rays = len(o)
    rows = []
    with capi.DeviceScene(fs, 0) as ds:
        ds.set_profiling(True)
        for tag, call in (("rr_render", lambda: ds.render(camc, cfg, aux=True)), ("rr_shade_rays", lambda: ds.shade_rays(o, d, cfg, spp))):
            call()                                   # first use: buffers grow
            best = None
            for _ in range(3):
                t0 = time.perf_counter(); out = call(); wall = (time.perf_counter() - t0) * 1e3
                st = ds.stats()
                if best is None or wall < best[0]:
                    best = (wall, st, out)
            rows.append((tag, best))
    print(f"{scene} {w}x{h}x{spp}: {n_rays} rays; per ray = ns")
    for tag, (wall, st, _) in rows:
        print(f"{tag:14s} host {wall:9.2f} ms  device {st['ms_total']:8.2f} ms  closest {st['ms_trace_closest']:7.2f} ms ({st['ms_trace_closest'] * 1e6 / n_rays:6.2f})  "
              f"shadow {st['ms_trace_shadow']:7.2f} ms ({st['ms_trace_shadow'] * 1e6 / n_rays:6.2f})  shade {st['ms_shade']:7.2f} ms ({st['ms_shade'] * 1e6 / n_rays:6.2f})  "
              f"batches {st['batches']}  rays p/s/sh {st['primary_rays']} / {st['secondary_rays']} / {st['shadow_rays']}")
    frame, got = rows[0][1][2], rows[1][1][2]
    b = (np.fmin(got["color"], np.float32(1.0)) * np.float32(255.0))
    b = np.where(np.isnan(b), 0, np.clip(np.floor(np.nan_to_num(b)), 0, 255)).astype(np.uint8)
    same = int((b == frame["rgba"].reshape(-1, 4)[:, :3]).all(axis=1).sum())
    print(f"pixels whose bytes equal the frame's: {same} of {w * h} (the rays here are numpy's, not primary_ray's: equal where the arithmetic agrees)")


if __name__ == "__main__":
    main()
