"""Raytracing::accumulate and Raytracing::accumulate_device of include/rustray_host.hpp, driven through host_shim.cpp: the records the
numpy yardstick gives, and a refusal of rr_accumulate_records coming back through the C++ layer."""
import ctypes as C

import numpy as np
import pytest

from rustray_amd import capi
from rustray_amd.flat import make_config
from rustray_amd.temporal import accumulate_records
from tests.denoise_cases import F
from tests.helpers import load_scene
from tests.temporal_cases import frame_params, temporal_frame
from tests.test_cpp_host import _cam_args
from tests.test_gpu_pixel_parts_cpp import _shim

pytestmark = pytest.mark.gpu

W, H = 37, 19
N = W * H


def test_accumulate_through_the_cpp_host_layer(hip):
    import torch
    case = temporal_frame(W, H)
    camera, prm = case["cam"], frame_params(case)
    want = accumulate_records(case["records"], case["halves"], case["history"], case["history_halves"], case["history_length"], case["motion"], camera, prm)
    first = accumulate_records(case["records"], None, None, None, None, None, camera, prm)
    fs = load_scene("spheres_room")
    cfg = make_config(samples=4, monte_carlo=True, seed=3, max_recursion=4)
    L = _shim()
    cam_types = list(L.rh_render_pixel_parts.argtypes[1:10])
    L.rh_accumulate_records.argtypes = [C.c_void_p] + cam_types + [C.c_void_p] * 11
    L.rh_accumulate_records_device.argtypes = [C.c_void_p] + cam_types + [C.c_void_p] * 12
    cs = fs.c_struct()
    h = L.rh_scene_create(C.byref(cs), 0)
    assert h
    args = _cam_args(camera) + (C.byref(cfg), W, H)
    P = lambda a: a.ctypes.data
    cprm = capi.accumulate_params(prm)
    try:
        out, out_h, length = np.zeros((N, 8), F), np.zeros((N, 2, 8), F), np.zeros(N, F)
        # (the C++ Camera forms its matrices from the same state as camera.Camera: the same rr_camera)
        assert L.rh_accumulate_records(h, *args, P(case["records"]), P(case["halves"]), P(case["history"]), P(case["history_halves"]), P(case["history_length"]),
                                       C.addressof(cprm), P(case["motion"]), P(out), P(out_h), P(length), None) == 0
        for got, key in ((out, "records"), (out_h, "halves"), (length, "length")):
            assert np.array_equal(got.view(np.uint32), want[key].view(np.uint32)), key
        # the first frame, one layer, the library's default parameters
        assert L.rh_accumulate_records(h, *args, P(case["records"]), None, None, None, None, None, None, P(out), None, P(length), None) == 0
        assert np.array_equal(out.view(np.uint32), first["records"].view(np.uint32)) and np.array_equal(length, first["length"])
        # the device form
        dev = {k: torch.from_numpy(np.ascontiguousarray(case[k]).copy()).cuda() for k in ("records", "halves", "history", "history_halves", "history_length", "motion")}
        d_out, d_out_h, d_len = torch.zeros((N, 8), device="cuda"), torch.zeros((N, 2, 8), device="cuda"), torch.zeros((N,), device="cuda")
        torch.cuda.synchronize()
        assert L.rh_accumulate_records_device(h, *args, C.addressof(cprm), *(dev[k].data_ptr() for k in ("records", "halves", "history", "history_halves",
                                                                                                        "history_length", "motion")),
                                              d_out.data_ptr(), d_out_h.data_ptr(), d_len.data_ptr(), None, None) == 0
        torch.cuda.synchronize()
        for got, key in ((d_out, "records"), (d_out_h, "halves"), (d_len, "length")):
            assert np.array_equal(got.cpu().numpy().view(np.uint32), want[key].view(np.uint32)), key
        # a refusal comes back through the layer
        cprm.snap = 0.5
        assert L.rh_accumulate_records(h, *args, P(case["records"]), None, None, None, None, C.addressof(cprm), None, P(out), None, P(length), None) == -1
        assert b"snap" in hip.lib().rr_last_error()
    finally:
        L.rh_scene_destroy(h)
