"""Edits of a live scene through rr_scene_update_lights, rr_scene_update_item_flags and rr_scene_add_textures: after each, the handle
renders bit for bit what a handle freshly created from the edited flat scene renders (all four buffers and the work counters), and
matches the oracle.  Refused and failing calls leave the scene as it was; calls from on_pass are refused; frames in flight finish on
the old scene; progressive, multi-handle, Raytracing.apply_scene and C++ host paths see the same edits.

Two scenes, as tests/test_gpu_scene_edits.py: kbert_room (8 items: every ray walks the top level) and a 42-item fuzzer scene (the
packet form of the top level; up to 32 enabled lights, fixed shadow slots at level 1).  Edited scenes are deep-copied from copies
that never went through c_struct() (its ctypes arrays do not deep-copy)."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

from rustray_amd import capi
from rustray_amd.flat import RR_LIGHT_POINT, RR_LIGHT_SPOT, Light, make_config, rr_config, rr_flat_scene, rr_frame, rr_light, rr_texture
from rustray_amd.renderer import RECREATE, Raytracing
from rustray_amd.scene import Scene
from tests.helpers import assert_frames_identical, assert_in_band, camera_for, compare_frames
from tests.test_gpu_scene_edits import EDIT_SCENES, edit_scene, frames_differ

pytestmark = pytest.mark.gpu

W, H = 72, 48
CFG = dict(samples=2, monte_carlo=True, seed=23)   # Monte Carlo: soft shadows jitter per light, on the light's own RNG stream
COUNTERS = ("primary_rays", "secondary_rays", "shadow_rays", "shaded_hits")


def _cam(fs, w=W, h=H):
    return camera_for(fs, w, h).c_struct()


def _counters(ds):
    st = ds.stats()
    return {k: st[k] for k in COUNTERS}


def _fresh(hip, cur, cam, cfg):
    """Frame and counters of a handle created from (a copy of) `cur`."""
    with hip.DeviceScene(copy.deepcopy(cur), 0) as fresh:
        return fresh.render(cam, cfg), _counters(fresh)


def _check_against_oracle(hip, ds, cur, oracle, cfg, what):
    """The edited handle against the oracle, at a small size: +-1 LSB, equal object ids and work counters."""
    cam = _cam(cur, 40, 24)
    got = ds.render(cam, cfg)
    st = ds.stats()
    keep = copy.deepcopy(cur)   # c_struct() borrows the copy's arrays: it must outlive the call
    ref = oracle.render(keep.c_struct(), cam, cfg, want_means=True, n_threads=8, want_counters=True)
    res = compare_frames(got, ref)
    assert res["n_rgb_over"] == 0 and res["n_id_diff"] == 0, (what, res)
    assert_in_band(res, what)
    c = ref["counters"]
    assert (st["primary_rays"], st["secondary_rays"], st["shaded_hits"]) == (c["rays_primary"], c["rays_secondary"], c["shaded_hits"]), what


def _fault(hip, point, kind, skip=0):
    L = hip.lib()
    L.rr_test_fault.argtypes = [C.c_char_p, C.c_int, C.c_int]
    assert L.rr_test_fault(point.encode(), kind, skip) == 0


def _centre(fs):
    return np.mean([np.asarray(it.trans, np.float64)[:3, 3] for it in fs.items], axis=0)


def light_steps(fs):
    """(name, scene) per step of the light sequence; each step starts from the one before."""
    cur = copy.deepcopy(fs)
    for k, l in enumerate(cur.lights):
        l.id = 1000 + k
    steps = []
    def brightest(skip=()):   # (kbert_room's light 0 is a directional light the room's walls shadow everywhere)
        return max((k for k, l in enumerate(cur.lights) if l.enabled and k not in skip), key=lambda k: (cur.lights[k].intensity, -k))
    i0 = brightest()
    l0 = cur.lights[i0]
    l0.intensity, l0.color, l0.pos = l0.intensity * 1.7, (0.9, 0.5, 0.2), tuple(np.asarray(l0.pos) + (0.5, 0.7, -0.3))
    steps.append(("edit", copy.deepcopy(cur)))
    j = brightest(skip=(i0,))
    cur.lights[j].enabled = False
    steps.append(("disable", copy.deepcopy(cur)))
    sc = Scene()                                      # Scene::add_default_light, with a light id from the scene's counter
    sc.item_id = 5000
    sc.lights = cur.lights
    sc.add_default_light()
    # ... moved next to the brightest light: where Scene::add_default_light puts it, kbert_room's walls hide it from every visible point
    cur.lights[-1].pos = tuple((np.asarray(l0.pos, np.float64) + (0.7, 0.3, 0.5)).tolist())
    steps.append(("add_default_light", copy.deepcopy(cur)))
    sc.delete_light_by_id(cur.lights[0].id)           # the later lights move up a slot: their RNG streams shift
    steps.append(("delete_light_0", copy.deepcopy(cur)))
    p = next(k for k, l in enumerate(cur.lights) if l.enabled and l.light_type == RR_LIGHT_POINT)
    lp = cur.lights[p]
    d = _centre(cur) - np.asarray(lp.pos, np.float64)
    lp.light_type, lp.dir, lp.max_angle = RR_LIGHT_SPOT, tuple((d / np.linalg.norm(d)).tolist()), 0.35
    steps.append(("point_to_spot", copy.deepcopy(cur)))
    cur.lights.clear()
    steps.append(("no_lights", copy.deepcopy(cur)))
    rng = np.random.default_rng(7)
    c = _centre(fs)
    for k in range(33):                               # 33 enabled lights: level 1 leaves the fixed shadow slots
        cur.lights.append(Light(pos=tuple((c + rng.uniform(-3.0, 3.0, 3) + (0.0, 4.0, 0.0)).tolist()), color=tuple(rng.uniform(0.3, 1.0, 3).tolist()),
                                intensity=float(rng.uniform(4.0, 12.0)), light_type=RR_LIGHT_POINT, id=2000 + k))
    steps.append(("33_lights", copy.deepcopy(cur)))
    del cur.lights[5:]
    steps.append(("back_to_5", copy.deepcopy(cur)))
    return steps


@pytest.mark.parametrize("name", EDIT_SCENES)
def test_light_sequence_equals_a_fresh_scene_and_the_oracle(hip, oracle, name):
    fs = edit_scene(name)
    work = copy.deepcopy(fs)
    cam, cfg = _cam(work), make_config(**CFG)
    with hip.DeviceScene(fs, 0) as ds:
        prev = ds.render(cam, cfg)
        for step, cur in light_steps(work):
            ds.update_lights(cur.lights)
            got = ds.render(cam, cfg)
            st = _counters(ds)
            assert frames_differ(got, prev), f"{step}: the edit does not change the frame, so it tests nothing"
            ref, ref_st = _fresh(hip, cur, cam, cfg)
            assert_frames_identical(got, ref, f"{step}: in place vs a fresh scene")
            assert st == ref_st, (step, st, ref_st)
            _check_against_oracle(hip, ds, cur, oracle, cfg, step)
            prev = got


def _coverage(fs, object_id):
    ids, counts = np.unique(np.asarray(object_id), return_counts=True)
    cover = dict(zip(ids.tolist(), counts.tolist()))
    return [cover.get(it.id, 0) for it in fs.items]


def _smooth(fs, it):
    m = fs.meshes[it.mesh]
    return fs.materials[it.material_cache].smooth_shading and len(m.normals) > 0 and len(m.normal_indices) > 0


def _flags(fs):
    return [it.visible for it in fs.items], [it.flip_normals for it in fs.items]


def _probe_rays(fs, n=256):
    rng = np.random.default_rng(3)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.repeat((_centre(fs) + (0.0, 0.5, 0.0))[None].astype(np.float32), n, axis=0)
    return o, d


def _same_queries(a, b, fs, cam):
    o, d = _probe_rays(fs)
    for x, y in zip(a.trace_rays(o, d), b.trace_rays(o, d)):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
    for px, py in ((W // 2, H // 2), (W // 4, H // 3), (3 * W // 4, 2 * H // 3)):
        assert bytes(a.pick(cam, px, py)) == bytes(b.pick(cam, px, py)), (px, py)


@pytest.mark.parametrize("name", EDIT_SCENES)
def test_item_flag_edits_equal_a_fresh_scene(hip, oracle, name):
    fs = edit_scene(name)
    work = copy.deepcopy(fs)
    cam, cfg = _cam(work), make_config(**CFG)
    with hip.DeviceScene(fs, 0) as ds:
        first = ds.render(cam, cfg)
        cover = _coverage(work, first["object_id"])
        order = sorted(range(len(work.items)), key=lambda i: (-cover[i], i))
        cur = copy.deepcopy(work)
        steps = []
        cur.items[order[0]].visible = False                        # the most visible item
        steps.append(("hide_most_visible", copy.deepcopy(cur)))
        flat = [i for i in order if cover[i] > 0 and cur.items[i].visible and cur.items[i].kind == 1 and not _smooth(cur, cur.items[i])]
        cur.items[flat[0]].flip_normals = True
        steps.append(("flip_flat", copy.deepcopy(cur)))
        smooth = [i for i in order if cover[i] > 0 and cur.items[i].visible and cur.items[i].kind == 1 and _smooth(cur, cur.items[i])]
        if smooth:                                                 # (kbert_room has no smooth-shaded mesh)
            cur.items[smooth[0]].flip_normals = True
            steps.append(("flip_smooth", copy.deepcopy(cur)))
        for it in cur.items:
            it.visible = False
        steps.append(("hide_all", copy.deepcopy(cur)))
        prev = first
        for step, s in steps:
            ds.update_item_flags(*_flags(s))
            got = ds.render(cam, cfg)
            st = _counters(ds)
            assert frames_differ(got, prev), f"{step}: the edit does not change the frame, so it tests nothing"
            ref, ref_st = _fresh(hip, s, cam, cfg)
            assert_frames_identical(got, ref, f"{step}: in place vs a fresh scene")
            assert st == ref_st, (step, st, ref_st)
            with hip.DeviceScene(copy.deepcopy(s), 0) as fresh:
                _same_queries(ds, fresh, s, cam)
            _check_against_oracle(hip, ds, s, oracle, cfg, step)
            prev = got
        # everything hidden: neither a pick nor a traced ray hits a hidden item
        found, item, face, toi = ds.trace_rays(*_probe_rays(work))
        assert not found.any()
        for px in range(0, W, 9):
            assert ds.pick(cam, px, H // 2).hit == 0
        assert (got["object_id"] == 0).all()
        # un-hiding everything gives the first frame back
        ds.update_item_flags(*_flags(work))
        assert_frames_identical(ds.render(cam, cfg), first, "flags of creation restored")
        # the item_host trap: a material update (unchanged materials) rebuilds the flag words from the host's copy of the items
        ds.update_item_flags(*_flags(steps[1][1]))
        edited = ds.render(cam, cfg)
        ds.update_materials(work.materials)
        assert_frames_identical(ds.render(cam, cfg), edited, "flags after a no-op material update")
        assert frames_differ(edited, first)


def _texture_target(fs, object_id):
    """The most visible item whose surface has texture coordinates (a sphere, or a mesh with uv faces)."""
    cover = _coverage(fs, object_id)
    ok = [k for k, it in enumerate(fs.items) if it.visible and cover[k] > 0 and (it.kind == 0 or len(fs.meshes[it.mesh].uv_indices) > 0)]
    return max(ok, key=lambda k: (cover[k], -k))


def _new_image(seed, w=16, h=8):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    img[..., 3] = 255
    return img


@pytest.mark.parametrize("name", EDIT_SCENES)
def test_added_textures_equal_a_fresh_scene_with_the_longer_list(hip, name):
    fs = edit_scene(name)
    work = copy.deepcopy(fs)
    cam, cfg = _cam(work), make_config(**CFG)
    n0 = len(work.textures)
    img, empty = _new_image(1), np.zeros((0, 0, 4), np.uint8)
    with hip.DeviceScene(fs, 0) as ds:
        f0 = ds.render(cam, cfg)
        i = _texture_target(work, f0["object_id"])
        edited = copy.deepcopy(work)
        edited.textures += [img, empty]
        m = edited.materials[edited.items[i].material]
        m.texture[0] = n0                                     # the new image as the base map of the most visible item
        other = next(k for k in range(len(edited.materials)) if k not in {it.material_cache for it in edited.items} and k != edited.items[i].material)
        edited.materials[other].texture[1] = n0 + 1            # the zero-size image: named, never sampled
        with pytest.raises(hip.RustrayHipError) as e:         # an index past the list: refused before the add
            ds.update_materials(edited.materials)
        assert e.value.code == -1
        assert ds.add_textures([img, empty]) == n0
        assert ds.add_textures([]) == n0 + 2                   # adding nothing changes nothing
        assert_frames_identical(ds.render(cam, cfg), f0, "after adding textures nobody names")
        ds.update_materials(edited.materials)                  # ... accepted after it
        got = ds.render(cam, cfg)
        assert frames_differ(got, f0)
        ref, ref_st = _fresh(hip, edited, cam, cfg)
        assert_frames_identical(got, ref, "added textures vs a fresh scene")
        assert _counters(ds) == ref_st
        past = copy.deepcopy(edited)
        past.materials[other].texture[1] = n0 + 2
        with pytest.raises(hip.RustrayHipError):
            ds.update_materials(past.materials)


def test_refused_calls_leave_the_scene_as_it_was(hip):
    fs = edit_scene("rich9110")
    work = copy.deepcopy(fs)
    cam, cfg = _cam(work), make_config(**CFG)
    L = hip.lib()
    n = len(work.items)
    with hip.DeviceScene(fs, 0) as ds:
        f0 = ds.render(cam, cfg)
        st0 = _counters(ds)

        def unchanged(what):
            assert_frames_identical(ds.render(cam, cfg), f0, what)
            assert _counters(ds) == st0, what
        bad = copy.deepcopy(work.lights)
        bad[1].light_type = 3
        with pytest.raises(hip.RustrayHipError) as e:
            ds.update_lights(bad)
        assert e.value.code == -1 and "light 1" in str(e.value)
        unchanged("bad light type")
        with pytest.raises(hip.RustrayHipError) as e:
            ds.update_item_flags([False] * (n - 1), [False] * (n - 1))
        assert e.value.code == -1
        unchanged("wrong n_items")
        ones = np.ones(n, np.uint8)
        p = ones.ctypes.data_as(C.c_void_p)
        assert L.rr_scene_update_item_flags(ds._h, None, p, n) == -1
        assert L.rr_scene_update_item_flags(ds._h, p, None, n) == -1
        assert L.rr_scene_update_lights(ds._h, None, 2) == -1
        first = C.c_uint32(77)
        assert L.rr_scene_add_textures(ds._h, None, 1, C.byref(first)) == -1
        one = (rr_texture * 1)()
        one[0].width, one[0].height, one[0].rgba8 = 2, 2, ones.ctypes.data
        assert L.rr_scene_add_textures(ds._h, one, 1, None) == -1
        unchanged("NULL arrays")
        nopix = (rr_texture * 2)()
        nopix[0].width, nopix[0].height, nopix[0].rgba8 = 2, 2, ones.ctypes.data
        nopix[1].width, nopix[1].height, nopix[1].rgba8 = 4, 4, None
        assert L.rr_scene_add_textures(ds._h, nopix, 2, C.byref(first)) == -1 and first.value == 77
        big = (rr_texture * 1)()
        big[0].width, big[0].height, big[0].rgba8 = 32769, 1, ones.ctypes.data   # refused before a pixel is read
        assert L.rr_scene_add_textures(ds._h, big, 1, C.byref(first)) == -2 and first.value == 77
        assert ds.add_textures([]) == len(work.textures)   # nothing was appended
        unchanged("refused textures")


def _edit_for(kind, work):
    """A scene edited by one call of `kind`, and the call that makes it."""
    e = copy.deepcopy(work)
    if kind == "lights":
        e.lights[0].intensity *= 0.3
        e.lights.append(Light(pos=tuple((_centre(work) + (1.0, 5.0, 1.0)).tolist()), intensity=60.0))   # one more: the buffer grows
        return e, lambda ds: ds.update_lights(e.lights)
    if kind == "item_flags":
        for it in e.items[::3]:
            it.visible = False
        return e, lambda ds: ds.update_item_flags(*_flags(e))
    e.textures.append(_new_image(5))
    e.materials[e.items[0].material].texture[0] = len(work.textures)
    return e, lambda ds: (ds.add_textures([e.textures[-1]]), ds.update_materials(e.materials))


POINTS = {"lights": "update_lights.device", "item_flags": "update_item_flags.device", "textures": "add_textures.device"}


@pytest.mark.parametrize("kind", list(POINTS))
@pytest.mark.parametrize("name", EDIT_SCENES)
def test_faults_leave_the_scene_as_it_was_or_refusing_frames(hip, name, kind):
    """One-shot faults (kinds 1-3) between the device write and the commit: the scene renders the old frame.  A sticky fault (4) fails
    the roll-back too: frame calls return RR_ERR_DEVICE until an update of the same kind succeeds.  add_textures writes nothing of the
    scene before its commit, so it has nothing to roll back and stays intact even then."""
    fs = edit_scene(name)
    work = copy.deepcopy(fs)
    cam, cfg = _cam(work), make_config(**CFG)
    edited, call = _edit_for(kind, work)
    with hip.DeviceScene(fs, 0) as ds:
        f0 = ds.render(cam, cfg)
        try:
            for k, code in ((1, -5), (2, -4), (3, -4)):
                _fault(hip, POINTS[kind], k)
                with pytest.raises(hip.RustrayHipError) as e:
                    call(ds)
                assert e.value.code == code, (k, str(e.value))
                assert_frames_identical(ds.render(cam, cfg), f0, f"after a failed {kind} update (kind {k})")
            _fault(hip, POINTS[kind], 4)
            with pytest.raises(hip.RustrayHipError) as e:
                call(ds)
            assert e.value.code == -5
        finally:
            _fault(hip, "", 0)
        if kind == "textures":
            assert_frames_identical(ds.render(cam, cfg), f0, "after a failed add_textures with a sticky fault")
        else:
            assert "rolling back failed too" in str(e.value)
            for attempt in (lambda: ds.render(cam, cfg), lambda: ds.pick(cam, W // 2, H // 2), lambda: ds.trace_rays(*_probe_rays(work, 4))):
                with pytest.raises(hip.RustrayHipError) as e:
                    attempt()
                assert e.value.code == -4 and "broken" in str(e.value)
            other = work.materials                                 # another kind of update does not mend it
            ds.update_materials(other)
            with pytest.raises(hip.RustrayHipError):
                ds.render(cam, cfg)
        call(ds)
        got = ds.render(cam, cfg)
        ref, _ = _fresh(hip, edited, cam, cfg)
        assert_frames_identical(got, ref, f"{kind} update after the faults vs a fresh scene")
        assert frames_differ(got, f0)


def reentry_child():
    """The body of the re-entry test, in a child process (a self-deadlock on the scene's lock becomes the parent's time limit)."""
    fs = edit_scene("kbert_room")
    work = copy.deepcopy(fs)
    cam, cfg = _cam(work), make_config(samples=4, monte_carlo=True, seed=2)
    L = capi.lib()
    lights = (rr_light * len(work.lights))(*[l.c_struct() for l in work.lights])
    n = len(work.items)
    flags = np.ones(n, np.uint8)
    img = _new_image(9)
    tex = (rr_texture * 1)()
    tex[0].width, tex[0].height, tex[0].rgba8 = img.shape[1], img.shape[0], img.ctypes.data
    with capi.DeviceScene(fs, 0) as ds:
        ref = ds.render(cam, cfg)
        seen = []

        def on_pass(user, done, total):
            first = C.c_uint32(0)
            for rc in (L.rr_scene_update_lights(ds._h, lights, len(work.lights)),
                       L.rr_scene_update_item_flags(ds._h, flags.ctypes.data_as(C.c_void_p), flags.ctypes.data_as(C.c_void_p), n),
                       L.rr_scene_add_textures(ds._h, tex, 1, C.byref(first))):
                seen.append((rc, L.rr_last_error().decode()))
            return 0
        out = {k: np.zeros_like(v) for k, v in ref.items()}
        fr = rr_frame(out["rgba"].ctypes.data, out["normal"].ctypes.data, out["depth"].ctypes.data, out["object_id"].ctypes.data)
        rc = L.rr_render_progressive(ds._h, C.byref(cam), C.byref(cfg), None, C.byref(fr), 4, capi.PASS_FN(on_pass), None, None)
        assert rc == 0, L.rr_last_error()
        assert len(seen) >= 6
        for rc_call, msg in seen:
            assert rc_call == -1 and "re-entry" in msg, (rc_call, msg)
        assert_frames_identical(out, ref, "the progressive frame")
        assert ds.add_textures([]) == len(work.textures)          # nothing was added from on_pass
    print("LIVE_REENTRY_OK", len(seen))


def test_calls_from_on_pass_are_refused(hip):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", "import tests.test_gpu_live_edits as t; t.reentry_child()"]
    try:
        r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        pytest.fail("the progressive frame did not finish within 120 s: an edit from on_pass deadlocked on the scene's lock")
    assert r.returncode == 0 and "LIVE_REENTRY_OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_frame_in_flight_finishes_on_the_old_scene(hip):
    """rr_render_region_device returns with the frame enqueued; an edit right after it must not change what that frame reads."""
    import torch
    from rustray_amd.flat import rr_region
    fs = edit_scene("rich9110")
    work = copy.deepcopy(fs)
    cam, cfg = _cam(work), make_config(**CFG)
    edited, _ = _edit_for("lights", work)
    flagged, _ = _edit_for("item_flags", work)
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
    with hip.DeviceScene(fs, 0) as ds:
        enqueue(ds)
        old = collect()
        enqueue(ds)
        ds.update_lights(edited.lights)                    # no synchronisation in between
        assert all(np.array_equal(a, b) for a, b in zip(collect(), old)), "the enqueued frame saw the new lights"
        enqueue(ds)
        lit = collect()
        enqueue(ds)
        ds.update_item_flags(*_flags(flagged))
        assert all(np.array_equal(a, b) for a, b in zip(collect(), lit)), "the enqueued frame saw the new item flags"
        with hip.DeviceScene(copy.deepcopy(edited), 0) as fresh:
            enqueue(fresh)
            fresh_lit = collect()
        assert all(np.array_equal(a, b) for a, b in zip(lit, fresh_lit))
        assert any(not np.array_equal(a, b) for a, b in zip(lit, old))


def test_progressive_and_multi_handle_frames_after_edits(hip):
    fs = edit_scene("rich9110")
    work = copy.deepcopy(fs)
    cam, cfg = _cam(work), make_config(**CFG)
    e, _ = _edit_for("lights", work)
    for it in e.items[1::4]:
        it.visible = False
    e.items[2].flip_normals = True
    e.textures.append(_new_image(11))
    e.materials[e.items[0].material].texture[0] = len(work.textures)
    ref, _ = _fresh(hip, e, cam, cfg)

    def edit(ds):
        ds.update_lights(e.lights)
        ds.update_item_flags(*_flags(e))
        assert ds.add_textures([e.textures[-1]]) == len(work.textures)
        ds.update_materials(e.materials)
    with hip.DeviceScene(fs, 0) as a, hip.DeviceScene(copy.deepcopy(work), 0) as b:
        f0 = a.render(cam, cfg)
        edit(a)
        edit(b)
        assert frames_differ(ref, f0)
        assert_frames_identical(a.render_progressive(cam, cfg, lambda *x: 0, min_passes=5, tiles=True), ref, "progressive tiles")
        assert_frames_identical(a.render_progressive(cam, cfg, lambda *x: 0, min_passes=2), ref, "progressive")
        assert_frames_identical(capi.render_multi([a, b], cam, cfg), ref, "rr_render_multi over two edited handles")


def test_apply_scene_goes_in_place_or_recreates(hip):
    fs = edit_scene("kbert_room")
    cur = copy.deepcopy(fs)
    camera = camera_for(cur, W, H)
    cfg = make_config(**CFG)
    rt = Raytracing(fs, camera)
    rt.config = cfg
    prev = rt.render_frame()

    def check(new, want):
        plan = rt.apply_scene(copy.deepcopy(new))
        assert plan == want, plan
        got = rt.render_frame()
        fresh = Raytracing(copy.deepcopy(new), camera)
        fresh.config = cfg
        assert_frames_identical(got, fresh.render_frame(), f"{want} vs a fresh Raytracing")
        fresh.close()
        return got
    cur.lights[1].intensity *= 2.0
    cur.lights[2].enabled = False
    got = check(cur, ["update_lights"])
    assert frames_differ(got, prev)
    cur.items[3].visible = False
    cur.items[5].flip_normals = True
    got2 = check(cur, ["update_item_flags"])
    assert frames_differ(got2, got)
    cur.textures.append(_new_image(13))
    cur.materials[cur.items[_texture_target(cur, got2["object_id"])].material].texture[0] = len(cur.textures) - 1
    got3 = check(cur, ["add_textures", "update_materials"])
    assert frames_differ(got3, got2)
    del cur.items[4]                                         # object "delete": the item count changes
    handle = rt.device_scene
    check(cur, [RECREATE])
    assert rt.device_scene is not handle
    assert check(cur, []) is not None                         # nothing left to do
    rt.close()


SHIM = os.path.join(os.path.dirname(capi.LIB_PATH), "librustray_host_shim.so")


def test_cpp_host_edits_equal_the_c_abi(hip):
    """DeviceScene / Raytracing edits of include/rustray_host.hpp, driven through host_shim.cpp: a light edit and a flag edit give the
    frame the same edits give through the C ABI (and a fresh scene)."""
    from tests.test_cpp_host import _cam_args
    assert os.path.exists(SHIM), f"{SHIM} is missing: run `make -C rustray_amd/csrc`"
    L = C.CDLL(SHIM)
    F3 = C.c_float * 3
    L.rh_scene_create.restype = C.c_void_p
    L.rh_scene_create.argtypes = [C.POINTER(rr_flat_scene), C.c_int]
    L.rh_scene_destroy.argtypes = [C.c_void_p]
    L.rh_update_lights.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    L.rh_update_item_flags.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    L.rh_add_textures.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    L.rh_scene_render.argtypes = [C.c_void_p, C.c_float, F3, F3, F3, C.c_float, C.c_float, C.POINTER(rr_config),
                                  C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    fs = edit_scene("rich9110")
    work = copy.deepcopy(fs)
    camera = camera_for(work, W, H)
    cam, cfg = camera.c_struct(), make_config(**CFG)
    e, _ = _edit_for("lights", work)
    e.items[0].visible = False
    e.items[1].flip_normals = True

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
        lights = (rr_light * len(e.lights))(*[l.c_struct() for l in e.lights])
        assert L.rh_update_lights(h, lights, len(e.lights)) == 0
        vis, flip = (np.asarray(a, np.uint8) for a in _flags(e))
        assert L.rh_update_item_flags(h, vis.ctypes.data, flip.ctypes.data, len(vis)) == 0
        assert L.rh_update_item_flags(h, vis.ctypes.data, flip.ctypes.data, len(vis) - 1) != 0   # refused: wrong item count
        got = render_cpp(h)
        first = C.c_uint32(0)
        assert L.rh_add_textures(h, None, 0, C.byref(first)) == 0 and first.value == len(work.textures)
    finally:
        L.rh_scene_destroy(h)
    with hip.DeviceScene(copy.deepcopy(work), 0) as ds:
        ds.update_lights(e.lights)
        ds.update_item_flags(*_flags(e))
        via_abi = ds.render(cam, cfg)
    assert frames_differ(got, f0)
    assert_frames_identical(got, via_abi, "C++ host edits vs the same edits through the C ABI")
    assert_frames_identical(got, _fresh(hip, e, cam, cfg)[0], "C++ host edits vs a fresh scene")
