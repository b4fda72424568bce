#!/usr/bin/env python3
"""Developer tool: host wall time per call of the four ray queries in their host form (rr_trace_rays, rr_trace_shadow_rays,
rr_shade_rays, rr_surface_rays: host arrays in, host arrays out) and in their device-buffer form (rr_trace_rays_device,
rr_trace_shadow_rays_device, rr_shade_rays_device, rr_surface_rays_device: inputs and outputs resident on the GPU as torch tensors,
the call followed by one synchronisation), on ONE
handle of scenes/spheres_room and about 1 Mi rays generated once: the primary rays of a 1024 x 1024 pinhole camera at the scene's
eye, the shadow rays from their hit points to the first point light (limit: the light's distance), the primaries again as
radiance rays (one per result, max_recursion 3) and as surface rays.  Median and minimum of 7 calls each, after one untimed call of each form.
usage: python tools/query_probe.py [side]      (default: 1024, i.e. 1 048 576 rays)"""
import ctypes as C
import os
import statistics
import sys
import time

import torch  # before the library: whichever HIP runtime a process loads first serves both (tests/conftest.py)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from rustray_amd import capi  # noqa: E402
from rustray_amd.flat import RR_LIGHT_DIRECTIONAL, FlatScene, make_config  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 7


def timed(fn):
    fn()                                               # first use: buffers grow, the top level is padded for these origins
    out = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out)


def main():
    side = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    n = side * side
    fs = FlatScene.load(os.path.join(ROOT, "scenes", "spheres_room.npz"))
    eye = np.asarray(fs.meta["camera"]["eye_pos"], np.float32)
    # a 90-degree pinhole looking down -z: un-normalised directions through the pixel centres, row-major
    u = ((np.arange(side, dtype=np.float32) + np.float32(0.5)) / np.float32(side) * np.float32(2.0) - np.float32(1.0)).astype(np.float32)
    d = np.stack([np.tile(u, side), np.repeat(-u, side), np.full(n, -1.0, np.float32)], axis=1).astype(np.float32)
    o = np.tile(eye[None, :], (n, 1)).astype(np.float32)
    cfg = make_config(samples=1, monte_carlo=True, seed=1, max_recursion=3)
    light = next(l for l in fs.lights if l.light_type != RR_LIGHT_DIRECTIONAL)
    with capi.DeviceScene(fs, 0) as ds:
        found, item, face, toi = ds.trace_rays(o, d, 1)
        hit = (o + d * np.where(found, toi, np.float32(1.0))[:, None]).astype(np.float32)
        to_light = (np.asarray(light.pos, np.float32)[None, :] - hit).astype(np.float32)
        dist = np.sqrt((to_light * to_light).sum(axis=1, dtype=np.float32)).astype(np.float32)
        so = (hit + to_light * np.float32(1e-3)).astype(np.float32)
        sd = (to_light / dist[:, None]).astype(np.float32)
        lim = (dist * np.float32(0.999)).astype(np.float32)
        dev = {k: torch.from_numpy(v).cuda() for k, v in dict(o=o, d=d, so=so, sd=sd, lim=lim).items()}
        out5 = torch.empty((n, 5), dtype=torch.int32, device="cuda")
        out8 = torch.empty((n, 8), dtype=torch.float32, device="cuda")
        out32 = torch.empty((n, 32), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()

        def dev_closest():
            ds.trace_rays_device(dev["o"].data_ptr(), dev["d"].data_ptr(), n, 1, out5.data_ptr())
            torch.cuda.synchronize()

        def dev_shadow():
            ds.trace_shadow_rays_device(dev["so"].data_ptr(), dev["sd"].data_ptr(), dev["lim"].data_ptr(), n, 1, out5.data_ptr())
            torch.cuda.synchronize()

        def dev_shade():
            ds.shade_rays_device(cfg, dev["o"].data_ptr(), dev["d"].data_ptr(), n, 1, None, out8.data_ptr())
            torch.cuda.synchronize()

        def dev_surface():
            ds.surface_rays_device(dev["o"].data_ptr(), dev["d"].data_ptr(), n, 1, out32.data_ptr())
            torch.cuda.synchronize()

        # the host forms through the C ABI itself, into arrays that exist: no binding work inside the clock
        L, vp = capi.lib(), C.c_void_p
        h5, h8, h32 = np.zeros((n, 5), np.uint32), np.zeros((n, 8), np.float32), np.zeros((n, 32), np.float32)

        def host_closest():
            capi._check(L.rr_trace_rays(ds._h, vp(o.ctypes.data), vp(d.ctypes.data), n, 1, vp(h5.ctypes.data)))

        def host_shadow():
            capi._check(L.rr_trace_shadow_rays(ds._h, vp(so.ctypes.data), vp(sd.ctypes.data), vp(lim.ctypes.data), n, 1,
                                               C.cast(h5.ctypes.data, C.POINTER(capi.rr_shadow_hit))))

        def host_shade():
            capi._check(L.rr_shade_rays(ds._h, C.byref(cfg), vp(o.ctypes.data), vp(d.ctypes.data), n, 1, None, vp(h8.ctypes.data), None))

        def host_surface():
            capi._check(L.rr_surface_rays(ds._h, vp(o.ctypes.data), vp(d.ctypes.data), n, 1, vp(h32.ctypes.data)))

        rows = (("closest hit", host_closest, dev_closest),
                ("shadow, limit = the light's distance", host_shadow, dev_shadow),
                ("radiance, max_recursion 3", host_shade, dev_shade),
                ("surface of the closest hit", host_surface, dev_surface))
        print(f"spheres_room, {len(fs.items)} items, {n} rays per call, median (min) of {REPS} calls, host wall time including the final synchronisation")
        for name, host_fn, dev_fn in rows:
            (hm, hl), (dm, dl) = timed(host_fn), timed(dev_fn)
            print(f"  {name:38s} host form {hm:9.3f} ({hl:9.3f}) ms   device form {dm:9.3f} ({dl:9.3f}) ms   host / device {hm / dm:6.1f}x   "
                  f"device form {dm * 1e6 / n:7.2f} ns per ray")


if __name__ == "__main__":
    main()
