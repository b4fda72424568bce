"""Raytracing::motion and Raytracing::motion_device of include/rustray_host.hpp, driven through host_shim.cpp: the words the C ABI and the
numpy yardstick give, and a refusal of rr_motion_records coming back through the C++ layer."""
import ctypes as C

import numpy as np
import pytest

from rustray_amd.flat import make_config
from rustray_amd.temporal import motion_records
from tests.denoise_cases import F, differing_words
from tests.motion_cases import motion_frame, motion_items, motion_scene, moved_list
from tests.test_cpp_host import _cam_args
from tests.test_gpu_pixel_parts_cpp import _shim

pytestmark = pytest.mark.gpu

W, H = 37, 19
N = W * H


def test_motion_through_the_cpp_host_layer(hip):
    import torch
    it, case = motion_items(), motion_frame(W, H)
    camera = case["cam"]
    idx, prev = moved_list(70)
    want = motion_records(case["records"], camera, it["ids"][idx], prev, it["trans_inv"][idx])
    prev_cm = np.ascontiguousarray(np.transpose(prev, (0, 2, 1)))
    fs = motion_scene()
    cfg = make_config(samples=4, monte_carlo=True, seed=3, max_recursion=4)
    L = _shim()
    cam_types = list(L.rh_render_pixel_parts.argtypes[1:10])
    L.rh_motion_records.argtypes = [C.c_void_p] + cam_types + [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rh_motion_records_device.argtypes = [C.c_void_p] + cam_types + [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    cs = fs.c_struct()
    h = L.rh_scene_create(C.byref(cs), 0)
    assert h
    args = _cam_args(camera) + (C.byref(cfg), W, H)
    P = lambda a: a.ctypes.data
    try:
        # (the C++ Camera forms its matrices from the same state as camera.Camera: the same rr_camera)
        motion, world = np.zeros((N, 3), F), np.zeros((N, 3), F)
        assert L.rh_motion_records(h, *args, P(idx), P(prev_cm), len(idx), P(case["records"]), P(motion), P(world)) == 0
        assert differing_words(motion, want[0]) == (0, 0) and differing_words(world, want[1])[0] == 0
        # the C ABI on the same handle's twin: the same words
        with hip.DeviceScene(fs, 0) as ds:
            abi_motion, abi_world = ds.motion_records(camera.c_struct(), idx, prev, case["records"], world=True)
        assert np.array_equal(motion.view(np.uint32), abi_motion.view(np.uint32)) and np.array_equal(world.view(np.uint32), abi_world.view(np.uint32))
        # without world_out, nothing moved
        only = np.ones((N, 3), F)
        assert L.rh_motion_records(h, *args, None, None, 0, P(case["records"]), P(only), None) == 0 and not only.any()
        # the device form
        rec = torch.from_numpy(case["records"].copy()).cuda()
        d_motion, d_world = torch.zeros((N, 3), device="cuda"), torch.zeros((N, 3), device="cuda")
        torch.cuda.synchronize()
        assert L.rh_motion_records_device(h, *args, P(idx), P(prev_cm), len(idx), rec.data_ptr(), d_motion.data_ptr(), d_world.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert np.array_equal(d_motion.cpu().numpy().view(np.uint32), motion.view(np.uint32)) and np.array_equal(d_world.cpu().numpy().view(np.uint32), world.view(np.uint32))
        # a refusal comes back through the layer
        twice = np.array([idx[0], idx[0]], np.uint32)
        assert L.rh_motion_records(h, *args, P(twice), P(prev_cm), 2, P(case["records"]), P(motion), None) == -1
        assert b"entries 0 and 1" in hip.lib().rr_last_error()
    finally:
        L.rh_scene_destroy(h)
