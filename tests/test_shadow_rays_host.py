"""rr_trace_shadow_rays without a device: the record's layout, the argument checks that come before anything touches the scene,
and the limit classes of the GPU tests (tests/shadow_ray_cases.py) on the oracle alone -- each class reaches the outcomes the GPU
tests then demand of the device."""
import ctypes as C
import os
import re

import numpy as np

from rustray_amd import capi
from tests import shadow_ray_cases as cases

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rustray_hip.h")


def test_record_is_twenty_bytes_and_matches_the_header():
    assert C.sizeof(capi.rr_shadow_hit) == 20
    text = open(HEADER).read()
    body = re.search(r"typedef struct rr_shadow_hit \{(.*?)\} rr_shadow_hit;", text, re.S).group(1)
    fields = re.findall(r"^\s*(uint32_t|float)\s+(\w+);", body, re.M)
    assert [(n, {"uint32_t": C.c_uint32, "float": C.c_float}[t]) for t, n in fields] == list(capi.rr_shadow_hit._fields_)
    assert "rr_trace_shadow_rays" in capi.EXPORTS


def test_argument_checks_that_need_no_device():
    L = capi.lib()
    o = np.zeros((2, 3), np.float32); d = np.ones((2, 3), np.float32)
    out = (capi.rr_shadow_hit * 2)()
    op, dp = o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p)
    never_read = C.create_string_buffer(64)   # stands for a scene: every check below returns before the handle is looked at
    scene = C.cast(never_read, C.c_void_p)
    assert L.rr_trace_shadow_rays(None, op, dp, None, 2, 1, out) == -1
    assert b"NULL" in L.rr_last_error()
    assert L.rr_trace_shadow_rays(None, None, None, None, 0, 1, None) == -1          # a NULL scene, even for no rays
    assert L.rr_trace_shadow_rays(scene, None, dp, None, 2, 1, out) == -1
    assert L.rr_trace_shadow_rays(scene, op, None, None, 2, 1, out) == -1
    assert L.rr_trace_shadow_rays(scene, op, dp, None, 2, 1, None) == -1
    assert L.rr_trace_shadow_rays(scene, None, None, None, 0, 1, None) == 0           # n == 0 touches nothing
    for depth in (0, 256):
        assert L.rr_trace_shadow_rays(scene, op, dp, None, 2, depth, out) == -1
        assert b"depth" in L.rr_last_error()
    assert L.rr_trace_shadow_rays(scene, op, dp, None, 0x7fffff01, 1, out) == -2       # refused before an array is read
    for bad in (float("nan"), -1.0):
        lim = np.array([0.0, bad], np.float32)
        assert L.rr_trace_shadow_rays(scene, op, dp, lim.ctypes.data_as(C.c_void_p), 2, 1, out) == -1
        assert b"max_distance[1]" in L.rr_last_error()


def test_limit_classes_reach_both_outcomes_on_the_oracle(oracle):
    fs, rays = cases.corner_case(oracle, "blocker")
    cls = cases.limit_classes(fs, rays)
    assert list(cls)[:7] == list(cases.FIXED_CLASSES) and "light0" in cls
    n_found = int(rays["found"].sum())
    assert n_found == 398 and len(rays["toi"]) > n_found
    for c in ("none", "t", "two_t", "1e30"):
        assert int(cases.expected_occluded(rays, cls[c]).sum()) == n_found
    for c in ("below_t", "half_t", "zero"):
        assert not cases.expected_occluded(rays, cls[c]).any()
    # the rays the blocker pass exists for: the first item lies beyond the light, none occluded
    assert not cases.expected_occluded(rays, cls["light0"]).any() and int((rays["found"] & (rays["toi"] > cls["light0"])).sum()) == 398
    fs, rays = cases.monkey_case(oracle)
    assert len(rays["toi"]) == 1902 and int(rays["found"].sum()) == 1467
    # a record that differs in any field is a mismatch; the oracle's own record is none
    exp = cases.expected_occluded(rays, None)
    own = (exp, np.where(exp, rays["item"], -1).astype(np.int32), np.where(exp, rays["face"], 0).astype(np.uint32), np.where(exp, rays["toi"], np.float32(0)).astype(np.float32))
    assert len(cases.mismatches(own, rays, None)) == 0
    wrong = (own[0], own[1], own[2] + np.uint32(1), own[3])
    assert len(cases.mismatches(wrong, rays, None)) == len(rays["toi"])
