#!/usr/bin/env python3
"""Developer tool: host wall time of the scene edits in place -- rr_scene_update_lights, rr_scene_update_item_flags,
rr_scene_add_textures, rr_scene_update_materials -- next to rr_scene_create of the same scene (median of several calls each; every
edit call waits for the device itself).
usage: python tools/edit_probe.py [scene]"""
import os
import statistics
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import copy  # noqa: E402

import numpy as np  # noqa: E402

import bench  # noqa: E402
from rustray_amd import capi  # noqa: E402
from rustray_amd.flat import Light  # noqa: E402


def ms(fn, reps):
    out = []
    for k in range(reps):
        t0 = time.perf_counter()
        fn(k)
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out)


scene = sys.argv[1] if len(sys.argv) > 1 else "sponza_syn"
fs, cam, cfg = bench.build_workload(scene, 1280, 720, 1, 1)
pristine = copy.deepcopy(fs)
create = ms(lambda k: capi.DeviceScene(copy.deepcopy(pristine), 0).close(), 3)
lights_a = list(pristine.lights)
lights_b = copy.deepcopy(lights_a)
for l in lights_b:
    l.intensity *= 0.5
more = lights_b + [Light(pos=(0.0, 5.0, 0.0), intensity=50.0)]
vis = [it.visible for it in pristine.items]
flip = [it.flip_normals for it in pristine.items]
hidden = [v if i % 7 else False for i, v in enumerate(vis)]
img = np.full((512, 512, 4), 128, np.uint8)
with capi.DeviceScene(fs, 0) as ds:
    ds.render(cam.c_struct(), cfg, aux=False)
    res = {
        "rr_scene_create": create,
        "rr_scene_update_lights": ms(lambda k: ds.update_lights(lights_a if k % 2 else lights_b), 11),
        "rr_scene_update_lights (one more light)": ms(lambda k: ds.update_lights(more if k % 2 else lights_a), 11),
        "rr_scene_update_item_flags": ms(lambda k: ds.update_item_flags(hidden if k % 2 else vis, flip), 11),
        "rr_scene_update_materials": ms(lambda k: ds.update_materials(pristine.materials), 11),
        "rr_scene_add_textures (512x512)": ms(lambda k: ds.add_textures([img]), 5),
    }
print(f"{scene}: {len(pristine.items)} items, {pristine.n_triangles_instanced()} instanced triangles, {len(pristine.lights)} lights, "
      f"{len(pristine.textures)} textures ({sum(t.shape[0] * t.shape[1] for t in pristine.textures) * 4 / 2**20:.1f} MiB)")
for k, (med, lo) in res.items():
    print(f"  {k:42s} median {med:9.3f} ms  min {lo:9.3f} ms")
