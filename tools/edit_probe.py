#!/usr/bin/env python3
"""Developer tool: host wall time of the scene edits in place -- rr_scene_update_lights, rr_scene_update_item_flags,
rr_scene_add_textures, rr_scene_update_materials -- next to rr_scene_create of the same scene, and of the structural edits --
rr_scene_set_items appending the reference's environment sphere, rr_scene_add_meshes + rr_scene_set_items appending its ground plane,
rr_scene_set_items deleting one mesh item from the middle -- each next to rr_scene_create of the edited scene (median of several
calls each; every edit call waits for the device itself).  The scene files of the two "add" actions are those of
tests/golden/add_objects.
usage: python tools/edit_probe.py [scene ...]      (default: sponza_syn lotus_syn)"""
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
from rustray_amd.scene import Scene, flat_scene_after_add  # noqa: E402

ADD_ROOT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "add_objects")


def ms(fn, reps):
    out = []
    for k in range(reps):
        t0 = time.perf_counter()
        fn(k)
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out)


def create_ms(flat, reps=3):
    copies = [copy.deepcopy(flat) for _ in range(reps)]   # (a handle keeps its flat scene's arrays: one copy per call, made outside the clock)
    return ms(lambda k: capi.DeviceScene(copies[k], 0).close(), reps)


def structural(ds, pristine):
    """The three structural edits on the live handle `ds` of `pristine`, each timed from the pristine item list (put back, untimed,
    between the calls) and next to rr_scene_create of the scene it leads to."""
    sphere = flat_scene_after_add(pristine, Scene.add_environment_sphere, ADD_ROOT)
    plane = flat_scene_after_add(pristine, Scene.add_ground_plane, ADD_ROOT)
    mid = [i for i, it in enumerate(pristine.items) if it.kind == 1]
    less = copy.deepcopy(pristine)
    del less.items[mid[len(mid) // 2]]
    n_meshes = len(pristine.meshes)
    assert ds.add_textures(sphere.textures[len(pristine.textures):]) == len(pristine.textures)   # the sphere's image: uploaded once, not timed

    def back():
        ds.set_items(pristine.items, pristine.materials)

    def add_plane(k):
        items = [copy.copy(it) for it in plane.items]
        items[-1].mesh = ds.add_meshes(plane.meshes[n_meshes:])   # (every call appends the two triangles again: meshes are never removed)
        ds.set_items(items, plane.materials)

    def timed(fn, reps=7):
        out = []
        for k in range(reps):
            t0 = time.perf_counter()
            fn(k)
            out.append((time.perf_counter() - t0) * 1e3)
            back()
        return statistics.median(out), min(out)
    return {
        "rr_scene_set_items (+ environment sphere)": timed(lambda k: ds.set_items(sphere.items, sphere.materials)),
        "  rr_scene_create with the sphere": create_ms(sphere),
        "rr_scene_add_meshes + set_items (+ ground plane)": timed(add_plane),
        "  rr_scene_create with the plane": create_ms(plane),
        "rr_scene_set_items (- one mesh item, middle)": timed(lambda k: ds.set_items(less.items, less.materials)),
        "  rr_scene_create without that item": create_ms(less),
    }


for scene in (sys.argv[1:] or ["sponza_syn", "lotus_syn"]):
    fs, cam, cfg = bench.build_workload(scene, 1280, 720, 1, 1)
    pristine = copy.deepcopy(fs)
    create = create_ms(pristine)
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
        }
        res.update(structural(ds, pristine))
        res["rr_scene_add_textures (512x512)"] = ms(lambda k: ds.add_textures([img]), 5)
    print(f"{scene}: {len(pristine.items)} items, {pristine.n_triangles_instanced()} instanced triangles, {len(pristine.lights)} lights, "
          f"{len(pristine.textures)} textures ({sum(t.shape[0] * t.shape[1] for t in pristine.textures) * 4 / 2**20:.1f} MiB)")
    for k, (med, lo) in res.items():
        print(f"  {k:50s} median {med:9.3f} ms  min {lo:9.3f} ms")
