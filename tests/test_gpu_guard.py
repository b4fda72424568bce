"""Nothing unwinds across the ABI, on the device path itself: the test-only fault hook makes the real entry
points throw -- on the calling thread, in a mesh-tree worker of rr_scene_create, in a device worker of rr_render_multi -- and every
call must come back with a status code, leave the handles usable and leak no device memory.  An update that fails part-way
leaves the scene rendering exactly what it rendered before the call."""
import ctypes as C

import numpy as np
import pytest

from rustray_amd import capi
from rustray_amd.flat import make_config
from tests.helpers import assert_frames_identical, camera_for, item_transforms, load_scene, with_transforms

pytestmark = pytest.mark.gpu


def _fault(point, kind, skip=0):
    L = capi.lib()
    L.rr_test_fault.argtypes = [C.c_char_p, C.c_int, C.c_int]
    assert L.rr_test_fault(point.encode(), kind, skip) == 0


def _free_bytes():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]


def test_scene_create_survives_exceptions_and_frees_what_it_holds():
    fs = load_scene("kbert_room")
    with capi.DeviceScene(fs, 0):
        pass   # first use of the device: runtime allocations settle
    free0 = _free_bytes()
    for point, kind, code in (("scene_create.host", 1, -5), ("scene_create.host", 2, -4), ("scene_create.mesh_worker", 1, -5),
                              ("scene_create.mesh_worker", 2, -4), ("scene_create.mesh_worker", 3, -4)):
        _fault(point, kind, 1 if "worker" in point else 0)
        with pytest.raises(capi.RustrayHipError) as e:
            capi.DeviceScene(fs, 0)
        assert e.value.code == code, (point, kind, str(e.value))
    _fault("", 0)
    assert abs(_free_bytes() - free0) < (8 << 20)
    with capi.DeviceScene(fs, 0) as ds:   # and the next create works
        cam = camera_for(fs, 64, 48).c_struct()
        assert ds.render(cam, make_config(samples=1, monte_carlo=False))["rgba"][..., 3].min() == 255


def test_frame_entry_points_survive_exceptions():
    fs = load_scene("kbert_room")
    cam = camera_for(fs, 96, 64).c_struct()
    cfg = make_config(samples=2, monte_carlo=True, seed=3)
    with capi.DeviceScene(fs, 0) as a, capi.DeviceScene(fs, 0) as b, capi.DeviceScene(fs, 0) as c:
        ref = a.render(cam, cfg)
        # a device worker of rr_render_multi throws: bad_alloc, then a runtime_error in the second worker to start
        for kind, skip, code in ((1, 0, -5), (2, 1, -4), (3, 2, -4)):
            _fault("render_multi.worker", kind, skip)
            with pytest.raises(capi.RustrayHipError) as e:
                capi.render_multi([a, b, c], cam, cfg)
            assert e.value.code == code and "device slot" in str(e.value)
        _fault("", 0)
        out = capi.render_multi([a, b, c], cam, cfg)   # every handle was unlocked and is usable
        assert np.array_equal(out["rgba"], ref["rgba"])
        # host vectors of rr_trace_rays and rr_scene_update_transforms
        o = np.zeros((16, 3), np.float32); d = np.tile(np.array([[0, 0, -1]], np.float32), (16, 1))
        _fault("trace_rays.host", 1)
        with pytest.raises(capi.RustrayHipError) as e:
            a.trace_rays(o, d)
        assert e.value.code == -5 and "rr_trace_rays" in str(e.value)
        a.trace_rays(o, d)
        t = np.stack([np.asarray(it.trans, np.float32) for it in fs.items])
        ti = np.stack([np.asarray(it.trans_inv, np.float32) for it in fs.items])
        _fault("update_transforms.host", 2)
        with pytest.raises(capi.RustrayHipError) as e:
            a.update_transforms(t, ti)
        assert e.value.code == -4
        _fault("", 0)
        a.update_transforms(t, ti)
        assert np.array_equal(a.render(cam, cfg)["rgba"], ref["rgba"])


@pytest.mark.parametrize("name", ["kbert_room", "rich9110"])
def test_transform_update_failing_part_way_leaves_the_scene_as_it_was(name):
    """Faults after the items' upload (before the flat normals are derived again) and after the top level's rebuild (before its
    upload): the update returns the fault's code, the next frame equals the frame of before bit for bit, and the next update works."""
    from tests.test_gpu_scene_edits import EDIT_CFG, edit_scene
    fs = edit_scene(name)
    cam = camera_for(fs, 72, 48).c_struct()
    cfg = make_config(**EDIT_CFG)
    t0, ti0 = item_transforms(fs)
    t, ti = item_transforms(fs, 3.0)
    moved_fs = with_transforms(fs, t, ti)   # (before fs.c_struct(): its ctypes arrays do not deep-copy)
    with capi.DeviceScene(fs, 0) as ds, capi.DeviceScene(moved_fs, 0) as fresh:
        f0 = ds.render(cam, cfg)
        moved = fresh.render(cam, cfg)
        assert not np.array_equal(moved["rgba"], f0["rgba"])
        try:
            for point in ("update_transforms.derive", "update_transforms.upload_tlas"):
                for kind, code in ((1, -5), (2, -4)):
                    what = f"{point} kind {kind}"
                    _fault(point, kind)
                    with pytest.raises(capi.RustrayHipError) as e:
                        ds.update_transforms(t, ti)
                    assert e.value.code == code, (what, str(e.value))
                    assert_frames_identical(ds.render(cam, cfg), f0, f"after a fault at {what}")
                    ds.update_transforms(t, ti)
                    assert_frames_identical(ds.render(cam, cfg), moved, f"the update after a fault at {what}")
                    ds.update_transforms(t0, ti0)
                    assert_frames_identical(ds.render(cam, cfg), f0, f"back after a fault at {what}")
        finally:
            _fault("", 0)


def test_far_camera_rebuild_failing_before_its_upload_is_redone():
    """A failed top-level rebuild for a far camera returns a code, and the next frames from that camera and from the near one are right.
    (The reach is now recorded only with the upload; recorded before it, as it was, the next far frame skips the rebuild and walks boxes
    padded for the near camera -- which at this scene and camera still yields the same frame, so this guards the error path only.)"""
    from rustray_amd.camera import Camera
    fs = load_scene("spheres")
    near = camera_for(fs, 64, 48).c_struct()
    st = dict(fs.meta["camera"]); st["width"], st["height"] = 64, 48
    d = np.asarray(st["dir"], np.float64); d /= np.linalg.norm(d)
    st["eye_pos"] = [float(v) for v in (np.asarray(st["eye_pos"], np.float64) - d * 3.0e6)]
    st["clipping_far"] = 1e7
    far = Camera.from_state(st).c_struct()
    cfg = make_config(samples=1, monte_carlo=False, seed=0, max_recursion=2)
    with capi.DeviceScene(fs, 0) as ds, capi.DeviceScene(fs, 0) as fresh:
        a0 = ds.render(near, cfg)
        want = fresh.render(far, cfg)
        try:
            for kind, code in ((1, -5), (2, -4)):
                _fault("tlas_reach.upload", kind)
                with pytest.raises(capi.RustrayHipError) as e:
                    ds.render(far, cfg)
                assert e.value.code == code, str(e.value)
                assert_frames_identical(ds.render(far, cfg), want, f"the far frame after a failed rebuild (kind {kind})")
                assert_frames_identical(ds.render(near, cfg), a0, f"back near (kind {kind})")
        finally:
            _fault("", 0)


@pytest.mark.parametrize("what", ["transforms", "materials"])
def test_update_whose_rollback_fails_leaves_a_scene_that_refuses_frames(what):
    """A fault that stays armed fails the update and then its rollback, which crosses the same point: the scene is marked broken,
    every frame call says so instead of rendering a mix of two scenes, and an update of the same kind that succeeds clears the mark."""
    import copy
    fs = load_scene("kbert_room")
    edited = copy.deepcopy(fs)
    for it in edited.items:
        edited.materials[it.material_cache].alpha = edited.materials[it.material].alpha = 0.0
    cam = camera_for(fs, 72, 48).c_struct()
    cfg = make_config(samples=2, monte_carlo=True, seed=11)
    t0, ti0 = item_transforms(fs)
    t, ti = item_transforms(fs, 3.0)
    o = np.zeros((4, 3), np.float32); d = np.tile(np.array([[0, 0, -1]], np.float32), (4, 1))
    with capi.DeviceScene(fs, 0) as ds:
        f0 = ds.render(cam, cfg)
        try:
            if what == "transforms":
                _fault("update_transforms.derive", 4)      # bad_alloc, stays armed
                with pytest.raises(capi.RustrayHipError) as e:
                    ds.update_transforms(t, ti)
                assert e.value.code == -5
            else:
                _fault("update_materials.device", 5)       # runtime_error, stays armed
                with pytest.raises(capi.RustrayHipError) as e:
                    ds.update_materials(edited.materials)
                assert e.value.code == -4
            assert "rolling back failed" in str(e.value), str(e.value)
        finally:
            _fault("", 0)
        for call in (lambda: ds.render(cam, cfg), lambda: ds.render_progressive(cam, cfg, lambda *a: False, min_passes=2, tiles=True),
                     lambda: ds.pick(cam, 36, 24), lambda: ds.trace_rays(o, d)):
            with pytest.raises(capi.RustrayHipError) as e:
                call()
            assert e.value.code == -4 and "broken" in str(e.value), str(e.value)
        if what == "transforms":
            ds.update_materials(fs.materials)                  # an update of the other kind does not clear the mark
            with pytest.raises(capi.RustrayHipError):
                ds.render(cam, cfg)
            ds.update_transforms(t0, ti0)
        else:
            ds.update_transforms(t0, ti0)
            with pytest.raises(capi.RustrayHipError):
                ds.render(cam, cfg)
            ds.update_materials(fs.materials)
        assert_frames_identical(ds.render(cam, cfg), f0, f"after a successful {what} update")
