"""Structural edits of a live scene through rr_scene_add_meshes and rr_scene_set_items (with rr_scene_add_textures): items deleted, the
reference's ground plane and environment sphere added (tests/golden/add_objects), resident meshes instanced again, the item order
reversed, the list emptied and restored.  After every step the handle renders bit for bit what a handle freshly created from the
edited flat scene renders (all four buffers and the work counters), answers rr_pick and rr_trace_rays as that handle does, and matches
the oracle at 40x24.  The sequences cross 16/17 and 512/513 items (the packet form of the top level, fixed shadow slots) and walk a
small scene from 2 to 14 items and back (the top level's share of the traversal stack changes at every step: the per-mesh trees are
rebuilt).  Refused and failing calls leave the scene as it was; calls from on_pass are refused; frames in flight finish on the old
scene; progressive, multi-handle, Raytracing.apply_scene(structural=True) and C++ host paths see the same edits.

"The frame differs from the step before" holds for every step but two, which cannot change a frame by construction and are held to
more instead: a reversed item order (the frame must be bit for bit the one before, and rr_trace_rays must name the mirrored item
indices), and kbert_room's ground plane, which lies in the plane of the room's floor and is hidden by it and the walls (the frame
must be the one before, and rays that go down outside the room must now end on the plane)."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

from rustray_amd import capi
from rustray_amd.flat import make_config, rr_config, rr_flat_scene, rr_frame, rr_item, rr_material, rr_mesh
from rustray_amd.renderer import RECREATE, Raytracing
from rustray_amd.scene import Scene
from tests.helpers import assert_frames_identical, camera_for
from tests.packet_pad import pad_inert
from tests.structural_steps import Live, coverage, flat_add, marker_ball, structural_steps
from tests.test_gpu_live_edits import CFG, H, W, _cam, _check_against_oracle, _counters, _fault, _flags
from tests.test_gpu_scene_edits import EDIT_SCENES, edit_scene, frames_differ
from tests.test_structural_edits_host import scene_of

pytestmark = pytest.mark.gpu

SAME_FRAME_STEPS = {("kbert_room", "add_ground_plane"), ("kbert_room", "reversed"), ("rich9110", "reversed")}


def _probes(work, n=256):
    """Rays for rr_trace_rays that stay the same over a sequence: from the unedited scene's centre in seeded directions, and straight
    down from a ring far outside it (what only an added ground plane stops)."""
    rng = np.random.default_rng(3)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    c = np.mean([np.asarray(it.trans, np.float64)[:3, 3] for it in work.items], axis=0) + (0.0, 0.5, 0.0)
    o = np.repeat(c[None].astype(np.float32), n, axis=0)
    a = np.linspace(0.0, 2.0 * np.pi, 16, endpoint=False)
    ring = np.stack([c[0] + 900.0 * np.cos(a), np.full(16, c[1] + 50.0), c[2] + 900.0 * np.sin(a)], axis=1).astype(np.float32)
    down = np.repeat(np.asarray([[0.0, -1.0, 0.0]], np.float32), 16, axis=0)
    return np.concatenate([o, ring]), np.concatenate([d, down])


def _queries(ds, work, cam):
    """What a handle answers to the probe rays and to three picks, as bytes."""
    o, d = _probes(work)
    parts = [np.ascontiguousarray(x).view(np.uint8).tobytes() for x in ds.trace_rays(o, d)]
    parts += [bytes(ds.pick(cam, px, py)) for px, py in ((W // 2, H // 2), (W // 4, H // 3), (3 * W // 4, 2 * H // 3))]
    return parts


def _check_step(hip, oracle, live, cur, prev, work, cam, cfg, what, same_frame=False, with_oracle=True):
    """One step of a sequence: the live handle (already edited to `cur`) against the step before, a fresh handle and the oracle.
    prev = (frame, queries) of the step before; returns the same of this one."""
    got = live.ds.render(cam, cfg)
    st = _counters(live.ds)
    q = _queries(live.ds, work, cam)
    if same_frame:
        assert_frames_identical(got, prev[0], f"{what}: an edit that cannot change the frame")
        assert q != prev[1], f"{what}: neither the frame nor the queries show the edit, so the step tests nothing"
    else:
        assert frames_differ(got, prev[0]), f"{what}: the edit does not change the frame, so it tests nothing"
    with hip.DeviceScene(copy.deepcopy(cur), 0) as fresh:
        ref = fresh.render(cam, cfg)
        ref_st = _counters(fresh)
        assert_frames_identical(got, ref, f"{what}: in place vs a fresh scene")
        assert st == ref_st, (what, st, ref_st)
        assert q == _queries(fresh, work, cam), f"{what}: rr_trace_rays / rr_pick in place vs a fresh scene"
    if with_oracle:
        _check_against_oracle(hip, live.ds, cur, oracle, cfg, what)
    return got, q


@pytest.mark.parametrize("name", EDIT_SCENES)
def test_structural_sequence_equals_a_fresh_scene_and_the_oracle(hip, oracle, name):
    fs = edit_scene(name)
    work = copy.deepcopy(fs)
    cam, cfg = _cam(work), make_config(**CFG)
    with Live(hip, work) as live:
        first = live.ds.render(cam, cfg)
        prev = (first, _queries(live.ds, work, cam))
        steps = structural_steps(work, first["object_id"], go_to_16=name == "rich9110")
        if name == "rich9110":
            counts = [len(s.items) for _, s in steps]
            assert 16 in counts and 17 in counts and counts[0] >= 17
        for step, cur in steps:
            live.goto(cur)
            prev = _check_step(hip, oracle, live, cur, prev, work, cam, cfg, f"{name} {step}", same_frame=(name, step) in SAME_FRAME_STEPS)
            if step == "reversed":   # the mirrored indices: item i of the list before is item n - 1 - i now
                o, d = _probes(work)
                found, item, face, toi = live.ds.trace_rays(o, d)
                assert found.any()
                with hip.DeviceScene(copy.deepcopy(steps[[s for s, _ in steps].index("second_instance")][1]), 0) as before:
                    f0, i0, face0, toi0 = before.trace_rays(o, d)
                assert np.array_equal(found, f0) and np.array_equal(item[found], len(cur.items) - 1 - i0[found])
                assert np.array_equal(face[found], face0[found]) and np.array_equal(toi[found].view(np.uint32), toi0[found].view(np.uint32))
        # the counts of the last list are the ones the in-place updates expect now; the counts of creation are refused
        last = steps[-1][1]
        assert len(last.items) != len(work.items) and len(last.materials) != len(work.materials)
        for call in (lambda: live.ds.update_materials(work.materials), lambda: live.ds.update_item_flags(*_flags(work))):
            with pytest.raises(hip.RustrayHipError) as e:
                call()
            assert e.value.code == -1
        assert_frames_identical(live.ds.render(cam, cfg), prev[0], "after updates with the counts of creation were refused")
        edited = copy.deepcopy(last)
        for it in edited.items[::3]:
            it.visible = False
        edited.items[1].flip_normals = not edited.items[1].flip_normals
        for m in edited.materials[::2]:
            m.reflectivity, m.base_color = 0.3, (0.8, 0.5, 0.3)
        t = np.stack([np.asarray(it.trans, np.float64) for it in edited.items])
        t[:, 0, 3] += 0.25
        for it, m in zip(edited.items, t.astype(np.float32)):
            it.trans, it.trans_inv = m, np.linalg.inv(m.astype(np.float64)).astype(np.float32)
            it.trans_inv[3] = (0.0, 0.0, 0.0, 1.0)
        live.ds.update_materials(edited.materials)
        live.ds.update_item_flags(*_flags(edited))
        live.ds.update_transforms(np.stack([it.trans for it in edited.items]), np.stack([it.trans_inv for it in edited.items]))
        _check_step(hip, oracle, live, edited, prev, work, cam, cfg, f"{name}: material, flag and transform updates with the new counts")


def test_crossing_512_and_513_items(hip, oracle):
    """A scene padded with small inert spheres and quads: 513 items (the per-ray top level) -> 512 (the packet form) -> 513, by
    deleting and restoring the most visible real item."""
    base = edit_scene("kbert_room")
    work = pad_inert(base, 513, "scattered", seed=5)
    cam, cfg = _cam(work), make_config(**CFG)
    with Live(hip, work) as live:
        first = live.ds.render(cam, cfg)
        prev = (first, _queries(live.ds, work, cam))
        cover = coverage(work, first["object_id"])
        most = max(range(len(base.items)), key=lambda i: (cover[i], -i))
        less = copy.deepcopy(work)
        del less.items[most]
        assert len(less.items) == 512
        live.goto(less)
        prev = _check_step(hip, oracle, live, less, prev, work, cam, cfg, "513 -> 512 items")
        live.goto(work)
        got, _ = _check_step(hip, oracle, live, work, prev, work, cam, cfg, "512 -> 513 items")
        assert_frames_identical(got, first, "513 items again")


def test_the_stack_share_changes_at_every_step(hip, oracle):
    """2 -> 14 items, one at a time, then back in two jumps: the top level's share of the traversal stack differs between any two of
    2 .. 13 items, so every step rebuilds the trees of kbert_room's two large meshes for another depth (rr_scene_build.h: stack_shares)."""
    base = edit_scene("kbert_room")
    cam, cfg = _cam(base), make_config(**CFG)
    with hip.DeviceScene(copy.deepcopy(base), 0) as ds:
        cover = coverage(base, ds.render(cam, cfg)["object_id"])
    order = sorted(range(len(base.items)), key=lambda i: (-cover[i], i))
    big = [i for i in range(len(base.items)) if len(base.meshes[base.items[i].mesh].indices) > 1000]
    assert len(big) == 2
    start = copy.deepcopy(base)
    start.items = [base.items[i] for i in big]                          # the two large meshes alone: 35 levels for their trees
    camera = camera_for(base, W, H)
    eye = np.asarray(camera.eye_pos, np.float64)
    towards = np.mean([np.asarray(it.trans, np.float64)[:3, 3] for it in start.items], axis=0) - eye
    with Live(hip, start) as live:
        first = live.ds.render(cam, cfg)
        prev = (first, _queries(live.ds, base, cam))
        cur, scenes = start, [start]
        rest = [i for i in order if i not in big]
        for k in range(12):
            if k < len(rest) and cover[rest[k]] > 0:
                nxt = copy.deepcopy(cur)
                nxt.items.append(copy.deepcopy(base.items[rest[k]]))
            else:
                nxt = marker_ball(cur, eye, towards, k, 9000 + k, 0.35)
            cur = nxt
            scenes.append(cur)
            live.goto(cur)
            prev = _check_step(hip, oracle, live, cur, prev, base, cam, cfg, f"{len(cur.items)} items")
        assert len(cur.items) == 14
        for n in (7, 2):
            live.goto(scenes[n - 2])
            prev = _check_step(hip, oracle, live, scenes[n - 2], prev, base, cam, cfg, f"back to {n} items")
        assert_frames_identical(prev[0], first, "2 items again")


def _plane_and_sphere(work):
    return flat_add(flat_add(work, Scene.add_ground_plane), Scene.add_environment_sphere)


def _c_items(live, new):
    items, _ = live.resident_items(new)
    keep = copy.deepcopy(new)
    keep.items = items
    c = keep.c_struct()
    return keep, c


def test_refused_calls_leave_the_scene_as_it_was(hip):
    fs = edit_scene("rich9110")
    work = copy.deepcopy(fs)
    cam, cfg = _cam(work), make_config(**CFG)
    L = hip.lib()
    with Live(hip, work) as live:
        ds = live.ds
        f0 = ds.render(cam, cfg)
        st0 = _counters(ds)

        def unchanged(what):
            assert_frames_identical(ds.render(cam, cfg), f0, what)
            assert _counters(ds) == st0, what

        def refused(edit, code, text, n_items=None):
            bad = copy.deepcopy(work)
            edit(bad)
            keep, c = _c_items(live, bad)
            rc = L.rr_scene_set_items(ds._h, c.items, len(bad.items) if n_items is None else n_items, c.materials, len(bad.materials))
            assert rc == code and text in L.rr_last_error().decode(), (rc, L.rr_last_error())
        keep, c = _c_items(live, work)
        n, nm = len(work.items), len(work.materials)
        assert L.rr_scene_set_items(ds._h, None, n, c.materials, nm) == -1
        assert L.rr_scene_set_items(ds._h, c.items, n, None, nm) == -1
        first = C.c_uint32(77)
        assert L.rr_scene_add_meshes(ds._h, None, 1, C.byref(first)) == -1 and L.rr_scene_add_meshes(ds._h, c.meshes, 1, None) == -1 and first.value == 77
        unchanged("NULL arrays")
        refused(lambda s: setattr(s.items[3], "kind", 5), -1, "item 3: kind 5")
        refused(lambda s: setattr(s.items[4], "material", len(s.materials)), -1, "item 4: material index")
        refused(lambda s: setattr(s.items[4], "material_cache", -1), -1, "item 4: material index")
        mesh_item = next(i for i, it in enumerate(work.items) if it.kind == 1)
        bad = copy.deepcopy(work)
        bad.items[mesh_item].mesh = len(live.meshes)                       # (past the resident meshes: not remapped, set directly)
        cb = bad.c_struct()
        assert L.rr_scene_set_items(ds._h, cb.items, n, cb.materials, nm) == -1 and f"item {mesh_item}: mesh index" in L.rr_last_error().decode()
        refused(lambda s: setattr(s.items[2], "material_cache", s.items[next(i for i, it in enumerate(s.items) if any(t >= 0 for t in s.materials[it.material].texture))].material),
                -1, "material_cache must not carry textures")
        refused(lambda s: s.materials[0].texture.__setitem__(2, len(s.textures)), -1, "material 0 texture slot 2")

        def nan_matrix(s):
            s.items[5].trans = np.asarray(s.items[5].trans, np.float32).copy()
            s.items[5].trans[1, 2] = np.nan
        refused(nan_matrix, -1, "item 5: non-finite transform")
        refused(lambda s: None, -2, "27 bits", n_items=1 << 27)             # refused before an item is read
        refused(lambda s: None, -2, "RR_MAX_ITEMS", n_items=(1 << 20) + 1)
        unchanged("refused item lists")
        # meshes: checked as rr_scene_create checks them, named by the index they would get
        m = (rr_mesh * 1)()
        pos = np.zeros((3, 3), np.float32)
        idx = np.asarray([[0, 1, 3]], np.uint32)
        m[0].positions, m[0].indices, m[0].n_vertices, m[0].n_triangles = pos.ctypes.data, idx.ctypes.data, 3, 1
        assert L.rr_scene_add_meshes(ds._h, m, 1, C.byref(first)) == -1 and first.value == 77
        assert f"mesh {len(work.meshes)}: vertex index 3" in L.rr_last_error().decode()
        assert ds.add_meshes([]) == len(work.meshes)                       # nothing was appended; adding nothing changes nothing
        unchanged("refused meshes")


@pytest.mark.parametrize("name", EDIT_SCENES)
def test_faults_leave_the_scene_as_it_was(hip, name):
    """Faults of kinds 1-3 (one shot) and 4 (sticky) at add_meshes.device and set_items.device, after the new state's upload and before
    the commit: the old frame and counters, no broken scene, and the same call then succeeds."""
    fs = edit_scene(name)
    work = copy.deepcopy(fs)
    cam, cfg = _cam(work), make_config(**CFG)
    edited = _plane_and_sphere(work)
    del edited.items[1]
    with Live(hip, work) as live:
        ds = live.ds
        f0 = ds.render(cam, cfg)
        st0 = _counters(ds)
        n_meshes = len(live.meshes)
        assert ds.add_textures(edited.textures[live.n_textures:]) == live.n_textures
        live.n_textures = len(edited.textures)
        items, appended = live.resident_items(edited)
        assert len(appended) == 1
        try:
            for point, call in (("add_meshes.device", lambda: ds.add_meshes(appended)), ("set_items.device", lambda: ds.set_items(items, edited.materials))):
                for kind, code in ((1, -5), (2, -4), (3, -4), (4, -5)):
                    _fault(hip, point, kind)
                    with pytest.raises(hip.RustrayHipError) as e:
                        call()
                    assert e.value.code == code, (point, kind, str(e.value))
                    _fault(hip, "", 0)
                    assert "rolling back" not in str(e.value)
                    assert_frames_identical(ds.render(cam, cfg), f0, f"after a fault of kind {kind} at {point}")
                    assert _counters(ds) == st0
                    assert ds.add_meshes([]) == n_meshes
                if point == "add_meshes.device":
                    assert ds.add_meshes(appended) == n_meshes             # the same call then succeeds
                    n_meshes += 1
                    assert_frames_identical(ds.render(cam, cfg), f0, "meshes nobody names")
                else:
                    call()
        finally:
            _fault(hip, "", 0)
        got = ds.render(cam, cfg)
        assert frames_differ(got, f0)
        with hip.DeviceScene(copy.deepcopy(edited), 0) as fresh:
            assert_frames_identical(got, fresh.render(cam, cfg), "the edit after the faults vs a fresh scene")
            assert _counters(ds) == _counters(fresh)


def reentry_child():
    """The body of the re-entry test, in a child process (a self-deadlock on the scene's lock becomes the parent's time limit)."""
    fs = edit_scene("kbert_room")
    work = copy.deepcopy(fs)
    cam, cfg = _cam(work), make_config(samples=4, monte_carlo=True, seed=2)
    L = capi.lib()
    keep = copy.deepcopy(work)
    c = keep.c_struct()
    with capi.DeviceScene(fs, 0) as ds:
        ref = ds.render(cam, cfg)
        seen = []

        def on_pass(user, done, total):
            first = C.c_uint32(0)
            for rc in (L.rr_scene_add_meshes(ds._h, c.meshes, 1, C.byref(first)),
                       L.rr_scene_set_items(ds._h, c.items, len(work.items) - 1, c.materials, len(work.materials))):
                seen.append((rc, L.rr_last_error().decode()))
            return 0
        out = {k: np.zeros_like(v) for k, v in ref.items()}
        fr = rr_frame(out["rgba"].ctypes.data, out["normal"].ctypes.data, out["depth"].ctypes.data, out["object_id"].ctypes.data)
        rc = L.rr_render_progressive(ds._h, C.byref(cam), C.byref(cfg), None, C.byref(fr), 4, capi.PASS_FN(on_pass), None, None)
        assert rc == 0, L.rr_last_error()
        assert len(seen) >= 4
        for rc_call, msg in seen:
            assert rc_call == -1 and "re-entry" in msg, (rc_call, msg)
        assert_frames_identical(out, ref, "the progressive frame")
        assert ds.add_meshes([]) == len(work.meshes)              # nothing was added from on_pass
        assert_frames_identical(ds.render(cam, cfg), ref, "the scene after the refused calls")
    print("STRUCTURAL_REENTRY_OK", len(seen))


def test_calls_from_on_pass_are_refused(hip):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", "import tests.test_gpu_structural_edits as t; t.reentry_child()"]
    try:
        r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        pytest.fail("the progressive frame did not finish within 120 s: an edit from on_pass deadlocked on the scene's lock")
    assert r.returncode == 0 and "STRUCTURAL_REENTRY_OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_frame_in_flight_finishes_on_the_old_scene(hip):
    """rr_render_region_device returns with the frame enqueued; an edit right after it must not change what that frame reads (the old
    buffers are released only after the device has finished it)."""
    import torch
    from rustray_amd.flat import rr_region
    fs = edit_scene("rich9110")
    work = copy.deepcopy(fs)
    cam, cfg = _cam(work), make_config(**CFG)
    edited = _plane_and_sphere(work)
    del edited.items[0]
    region = rr_region(32, 8, 1, 0)
    npx = W * H
    dev = torch.device("cuda", 0)
    bufs = [torch.zeros(npx * 4, dtype=torch.uint8, device=dev), torch.zeros(npx * 3, dtype=torch.float32, device=dev),
            torch.zeros(npx, dtype=torch.float32, device=dev), torch.zeros(npx, dtype=torch.int32, device=dev)]
    stream = torch.cuda.Stream(device=dev)

    def enqueue(ds):
        for b in bufs:
            b.fill_(0)
        torch.cuda.synchronize(dev)
        ds.render_region_device(cam, cfg, region, [b.data_ptr() for b in bufs], stream.cuda_stream)

    def collect():
        stream.synchronize()
        return [b.cpu().numpy().view(np.uint8).copy() for b in bufs]
    with Live(hip, work) as live:
        enqueue(live.ds)
        old = collect()
        assert live.ds.add_textures(edited.textures[live.n_textures:]) == live.n_textures
        live.n_textures = len(edited.textures)
        items, appended = live.resident_items(edited)
        enqueue(live.ds)
        live.ds.add_meshes(appended)                      # no synchronisation in between: the arenas are replaced
        assert all(np.array_equal(a, b) for a, b in zip(collect(), old)), "the enqueued frame saw the grown mesh arenas"
        enqueue(live.ds)
        live.ds.set_items(items, edited.materials)
        assert all(np.array_equal(a, b) for a, b in zip(collect(), old)), "the enqueued frame saw the new items"
        enqueue(live.ds)
        new = collect()
        with hip.DeviceScene(copy.deepcopy(edited), 0) as fresh:
            enqueue(fresh)
            fresh_new = collect()
        assert all(np.array_equal(a, b) for a, b in zip(new, fresh_new))
        assert any(not np.array_equal(a, b) for a, b in zip(new, old))


def test_progressive_and_multi_handle_frames_after_edits(hip):
    fs = edit_scene("rich9110")
    work = copy.deepcopy(fs)
    cam, cfg = _cam(work), make_config(**CFG)
    e = _plane_and_sphere(work)
    del e.items[2]
    e.items.reverse()
    with hip.DeviceScene(copy.deepcopy(e), 0) as fresh:
        ref = fresh.render(cam, cfg)
    with Live(hip, work) as a, Live(hip, work) as b:
        f0 = a.ds.render(cam, cfg)
        a.goto(e)
        b.goto(e)
        assert frames_differ(ref, f0)
        assert_frames_identical(a.ds.render_progressive(cam, cfg, lambda *x: 0, min_passes=5, tiles=True), ref, "progressive tiles")
        assert_frames_identical(a.ds.render_progressive(cam, cfg, lambda *x: 0, min_passes=2), ref, "progressive")
        assert_frames_identical(capi.render_multi([a.ds, b.ds], cam, cfg), ref, "rr_render_multi over two edited handles")


def test_apply_scene_structural_keeps_the_handle(hip):
    """Raytracing.apply_scene(..., structural=True) on flat scenes as Scene.flatten() lays them out (the material caches behind the full
    materials: one added item moves every cache index)."""
    cur = scene_of(edit_scene("kbert_room"))
    camera = camera_for(edit_scene("kbert_room"), W, H)
    cfg = make_config(**CFG)
    rt = Raytracing(cur.flatten(), camera)
    rt.config = cfg
    handle = rt.device_scene
    prev = rt.render_frame()

    def check(want, in_place=True):
        new = cur.flatten()
        plan = rt.apply_scene(copy.deepcopy(new), structural=True)
        assert plan == want, plan
        assert (rt.device_scene is handle) == in_place
        got = rt.render_frame()
        fresh = Raytracing(copy.deepcopy(new), camera)
        fresh.config = cfg
        assert_frames_identical(got, fresh.render_frame(), f"{want} vs a fresh Raytracing")
        assert _counters(rt.device_scene) == _counters(fresh.device_scene)
        fresh.close()
        return got
    cover = coverage(rt.flat_scene, prev["object_id"])
    cur.delete_object_by_id(rt.flat_scene.items[int(np.argmax(cover))].id)
    got = check(["set_items"])
    assert frames_differ(got, prev)
    cur.add_ground_plane()
    cur.lights[0].intensity *= 1.5
    got2 = check(["add_meshes", "set_items", "update_lights"])
    assert frames_differ(got2, got)
    cur.add_environment_sphere()
    got3 = check(["add_textures", "set_items"])
    assert frames_differ(got3, got2)
    cur.add_ground_plane()                                     # the plane's mesh is resident: no mesh is added for the second one
    check(["set_items"])
    cur.items[0].visible = False                                # nothing structural: the default plan
    got4 = check(["update_item_flags"])
    assert frames_differ(got4, got3)
    assert check([]) is not None
    cur.textures[0] = cur.textures[0].copy()
    cur.textures[0][..., 0] ^= 0x40                             # a resident image changed: a new handle
    cur.delete_object_by_id(cur.items[-1].id)
    check([RECREATE], in_place=False)
    assert rt.apply_scene(cur.flatten()) == []                  # the default mode, on the new handle
    rt.close()


SHIM = os.path.join(os.path.dirname(capi.LIB_PATH), "librustray_host_shim.so")


def test_cpp_host_edits_equal_the_c_abi(hip):
    """DeviceScene::add_meshes / set_items of include/rustray_host.hpp, driven through host_shim.cpp: the frame the same edits give
    through the C ABI (and a fresh scene)."""
    from tests.test_cpp_host import _cam_args
    assert os.path.exists(SHIM), f"{SHIM} is missing: run `make -C rustray_amd/csrc`"
    L = C.CDLL(SHIM)
    F3 = C.c_float * 3
    L.rh_scene_create.restype = C.c_void_p
    L.rh_scene_create.argtypes = [C.POINTER(rr_flat_scene), C.c_int]
    L.rh_scene_destroy.argtypes = [C.c_void_p]
    L.rh_add_textures.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    L.rh_add_meshes.argtypes = [C.c_void_p, C.POINTER(rr_mesh), C.c_uint32, C.POINTER(C.c_uint32)]
    L.rh_set_items.argtypes = [C.c_void_p, C.POINTER(rr_item), C.c_uint32, C.POINTER(rr_material), C.c_uint32]
    L.rh_scene_render.argtypes = [C.c_void_p, C.c_float, F3, F3, F3, C.c_float, C.c_float, C.POINTER(rr_config),
                                  C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    fs = edit_scene("rich9110")
    work = copy.deepcopy(fs)
    camera = camera_for(work, W, H)
    cam, cfg = camera.c_struct(), make_config(**CFG)
    e = flat_add(work, Scene.add_ground_plane)          # (the plane's mesh is the last of e.meshes, the others are those of creation, in order)
    del e.items[3]
    assert len(e.meshes) == len(work.meshes) + 1 and len(e.textures) == len(work.textures)

    def render_cpp(h):
        out = dict(rgba=np.zeros((H, W, 4), np.uint8), normal=np.zeros((H, W, 3), np.float32), depth=np.zeros((H, W), np.float32),
                   object_id=np.zeros((H, W), np.uint32))
        rc = L.rh_scene_render(h, *_cam_args(camera), C.byref(cfg), W, H, 3, *[out[k].ctypes.data for k in ("rgba", "normal", "depth", "object_id")])
        assert rc == 0
        return out
    cs = fs.c_struct()
    h = L.rh_scene_create(C.byref(cs), 0)
    assert h
    try:
        f0 = render_cpp(h)
        keep = copy.deepcopy(e)
        ce = keep.c_struct()
        first = C.c_uint32(0)
        new_mesh = C.cast(C.byref(ce.meshes[len(work.meshes)]), C.POINTER(rr_mesh))
        assert L.rh_add_meshes(h, new_mesh, 1, C.byref(first)) == 0 and first.value == len(work.meshes)
        assert L.rh_set_items(h, ce.items, len(e.items), ce.materials, len(e.materials) - 1) != 0    # refused: an item names the last material
        assert L.rh_set_items(h, ce.items, len(e.items), ce.materials, len(e.materials)) == 0
        got = render_cpp(h)
    finally:
        L.rh_scene_destroy(h)
    with Live(hip, work) as live:
        live.goto(e)
        via_abi = live.ds.render(cam, cfg)
    assert frames_differ(got, f0)
    assert_frames_identical(got, via_abi, "C++ host edits vs the same edits through the C ABI")
    with hip.DeviceScene(copy.deepcopy(e), 0) as fresh:
        assert_frames_identical(got, fresh.render(cam, cfg), "C++ host edits vs a fresh scene")
