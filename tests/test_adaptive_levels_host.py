"""Refinement level by level, without a GPU: adaptive.refine_sublist against a plain loop, the arithmetic the sublist kernels share with
the host (rustray_amd/csrc/rr_adaptive.h) under AddressSanitizer + UBSan on the CPU, and what rr_refine_sublist_device,
rr_render_adaptive_levels and rr_render_adaptive_levels_device refuse before they touch a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from rustray_amd import adaptive, capi
from rustray_amd.flat import make_config, rr_radiance
from tests.helpers import ROOT, host_api_source
from tests.test_pixel_parts import _camera

NEW = ("rr_refine_sublist_device", "rr_render_adaptive_levels", "rr_render_adaptive_levels_device")


def _loop(error, threshold, xy, count):
    out = []
    for i in range(count):
        if np.float32(error[i]) > np.float32(threshold):        # (False for NaN; the threshold is a binary32 number, as the library takes it)
            out.append(int(xy[i]))
    taken = len(out)
    while len(out) % 64:
        out.append(out[taken - 1])
    return np.array(out, np.uint32), taken


def _case(count, seed, own_pad=64):
    rng = np.random.default_rng(seed)
    xy = rng.integers(0, 2 ** 32, count + own_pad, dtype=np.uint64).astype(np.uint32)
    if count > 1:
        xy[1] = xy[0]                             # a duplicate is an entry like any other
    err = rng.choice(np.array([0.0, 0.05, 0.1, 0.25, 0.5, np.nan], np.float32), count + own_pad)
    err[count:] = 0.5                             # the list's own pad lies above every threshold below: it is never taken
    return xy, err


@pytest.mark.parametrize("count", (0, 1, 63, 64, 65, 200, 4097))
@pytest.mark.parametrize("threshold", (0.1, -1.0, 2.0))
def test_refine_sublist_against_a_plain_loop(count, threshold):
    xy, err = _case(count, 100 + count)
    got, taken = adaptive.refine_sublist(err, threshold, xy, count)
    want, want_taken = _loop(err, threshold, xy, count)
    assert got.dtype == np.uint32 and taken == want_taken and np.array_equal(got, want)
    assert len(got) == (taken + 63) // 64 * 64                        # padded to 64, and an empty result has no pad
    if taken:
        assert (got[taken:] == got[taken - 1]).all()
    if threshold < 0:
        assert taken == int((~np.isnan(err[:count])).sum())           # a negative threshold takes all `count` (half_error gives no NaN; one given here is not taken)
    if threshold > 1:
        assert taken == 0 and len(got) == 0


def test_refine_sublist_rules():
    xy = np.arange(10, dtype=np.uint32) + 1000
    err = np.array([0.5, 0.1, np.nan, 0.10000001, 0.0, 0.5, 0.5, 0.5, 0.5, 0.5], np.float32)
    got, taken = adaptive.refine_sublist(err, np.float32(0.1), xy, 5)
    assert taken == 2 and list(got[:2]) == [1000, 1003]               # order kept; error == threshold and NaN are not taken; entries 5 .. 9 neither
    assert len(got) == 64 and (got[2:] == 1003).all()
    got, taken = adaptive.refine_sublist(np.where(np.isnan(err), np.float32(0), err), -1.0, xy, 5)
    assert taken == 5 and list(got[:5]) == [1000, 1001, 1002, 1003, 1004]
    got, taken = adaptive.refine_sublist(err, 0.1, xy, 0)
    assert taken == 0 and len(got) == 0
    with pytest.raises(ValueError):
        adaptive.refine_sublist(err, 0.1, xy, 11)


def test_sublist_arithmetic_under_asan(tmp_path):
    exe = str(tmp_path / "adaptive_sublist_test")
    cmd = ["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-o", exe, os.path.join(ROOT, "tests", "native", "adaptive_sublist_test.cpp")]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "adaptive sublist test OK" in out.stdout, out.stdout + out.stderr


def _levels(*counts):
    return (C.c_uint16 * max(len(counts), 1))(*counts)


def test_fused_call_refusals_without_a_device():
    """Every call below is refused on its arguments alone, before the scene is looked at: the made-up handle is never dereferenced."""
    L = capi.lib()
    cam = _camera()
    n = 50 * 38
    cfg = make_config(samples=1)
    out = (rr_radiance * n)()
    C.memset(out, 0x5a, C.sizeof(out))
    out_p = C.cast(out, C.c_void_p)
    fake = C.c_void_p(0x1000)
    level_pixels = (C.c_uint32 * 8)(*([77] * 8))

    def host(levels=(6, 14, 30), n_levels=None, thr=0.1, o=out_p, camera=cam, scene=fake):
        lv = _levels(*levels)
        return L.rr_render_adaptive_levels(scene, C.byref(camera), C.byref(cfg), lv, len(levels) if n_levels is None else n_levels, thr, None, o, None, None, None,
                                           level_pixels, None)

    def device(levels=(6, 14, 30), n_levels=None, thr=0.1, o=out_p, camera=cam, scene=fake, samples=None, error=None, rgba=None):
        lv = _levels(*levels)
        return L.rr_render_adaptive_levels_device(scene, C.byref(camera), C.byref(cfg), lv, len(levels) if n_levels is None else n_levels, thr, None, o, rgba, samples,
                                                  error, level_pixels, None, None)

    for call in (host, device):
        for nl in (0, 1, 9):
            assert call(levels=(6, 8, 10, 12, 14, 16, 18, 20, 22), n_levels=nl) == -1
            assert b"n_levels" in L.rr_last_error() and str(nl).encode() in L.rr_last_error()
        for levels, at in (((7, 14, 30), 0), ((6, 15, 30), 1), ((6, 14, 31), 2), ((0, 14, 30), 0), ((6, 14, 0), 2)):      # odd counts, a count of 0
            assert call(levels=levels) == -1
            assert b"halves" in L.rr_last_error() and b"equal" in L.rr_last_error() and f"level_samples[{at}]".encode() in L.rr_last_error()
        for levels, at in (((6, 6, 30), 1), ((6, 14, 14), 2), ((6, 14, 12), 2), ((16, 6, 30), 1)):                       # equal or decreasing counts
            assert call(levels=levels) == -1
            assert f"level_samples[{at}]".encode() in L.rr_last_error() and b"increase strictly" in L.rr_last_error()
        assert call(levels=(6, 14, 16384)) == -2                    # rr_render's rule for the built-in table
        assert b"samples" in L.rr_last_error()
        assert call(thr=float("nan")) == -1
        assert b"NaN" in L.rr_last_error()
        assert call(o=None) == -1
        assert b"out" in L.rr_last_error()
        assert call(scene=None) == -1
        assert call(camera=_camera(0, 38)) == -1                    # width == 0
        assert call(camera=_camera(32768, 16385)) == -2             # 2 x 2^29 + 65536 slots: refused before anything is allocated
        assert b"2^30" in L.rr_last_error()
    # the device form's alignment rules
    assert device(o=C.c_void_p(C.addressof(out) + 8)) == -1
    assert b"aligned" in L.rr_last_error()
    assert device(samples=C.c_void_p(C.addressof(out) + 1)) == -1
    assert b"aligned" in L.rr_last_error()
    assert device(error=C.c_void_p(C.addressof(out) + 2)) == -1 and device(rgba=C.c_void_p(C.addressof(out) + 2)) == -1
    assert bytes(out) == b"\x5a" * C.sizeof(out) and list(level_pixels) == [77] * 8


def test_sublist_refusals_without_a_device():
    L = capi.lib()
    count_in = 100
    parts = (rr_radiance * (2 * 128))()
    C.memset(parts, 0x5a, C.sizeof(parts))
    parts_p = C.cast(parts, C.c_void_p)
    lst = np.full(128, 0x5a5a5a5a, np.uint32)
    lst_out = np.full(128, 0x5a5a5a5a, np.uint32)
    err = np.full(128, 0x5a5a5a5a, np.uint32)
    fake = C.c_void_p(0x1000)
    taken = C.c_uint32(77)

    def sub(lp=lst.ctypes.data, count=count_in, pp=parts_p, thr=0.1, ep=err.ctypes.data, op=lst_out.ctypes.data, cnt=C.byref(taken), scene=fake):
        return L.rr_refine_sublist_device(scene, C.c_void_p(lp) if lp else None, count, pp, thr, C.c_void_p(ep) if ep else None, C.c_void_p(op) if op else None, cnt, None)

    assert sub(lp=None) == -1 and b"list_dev" in L.rr_last_error()
    assert sub(pp=None) == -1 and b"parts_dev" in L.rr_last_error()
    assert sub(op=None) == -1 and b"list_out_dev" in L.rr_last_error()
    assert sub(cnt=None) == -1 and sub(scene=None) == -1
    assert sub(pp=C.c_void_p(C.addressof(parts) + 8)) == -1
    assert b"parts_dev" in L.rr_last_error() and b"aligned" in L.rr_last_error()
    assert sub(lp=lst.ctypes.data + 2) == -1 and b"aligned" in L.rr_last_error()
    assert sub(ep=err.ctypes.data + 2) == -1 and sub(op=lst_out.ctypes.data + 2) == -1
    # aliasing lists: the same buffer, the output's pad reaching into the input, the input's end reaching into the output
    assert sub(op=lst.ctypes.data) == -1 and b"overlaps" in L.rr_last_error()
    assert sub(lp=lst.ctypes.data + 4 * 60, count=28, op=lst.ctypes.data) == -1           # the output's pad, 64 entries in all, reaches entry 60
    assert b"overlaps" in L.rr_last_error()
    assert sub(lp=lst.ctypes.data, count=100, op=lst.ctypes.data + 4 * 99) == -1
    assert sub(count=(1 << 29) + 1) == -2 and b"2^29" in L.rr_last_error()
    assert sub(thr=float("nan")) == -1 and b"NaN" in L.rr_last_error()
    assert taken.value == 77
    # an empty list: RR_OK and a count of 0, with nothing launched (the made-up handle is not looked at) and no other pointer required
    assert sub(count=0) == 0 and taken.value == 0
    taken.value = 77
    assert sub(count=0, lp=None, pp=None, op=None, ep=None) == 0 and taken.value == 0
    assert bytes(parts) == b"\x5a" * C.sizeof(parts)
    for a in (lst, lst_out, err):
        assert (a == 0x5a5a5a5a).all()


def test_the_new_entry_points_are_guarded_and_bound():
    src = host_api_source()
    for n in NEW:
        assert re.search(r'^int ' + n + r'\([^{]*\) try \{', src, re.M), f"{n} is not a function-try-block"
        assert f'RR_GUARD_END("{n}")' in src
        assert n in capi.EXPORTS and hasattr(capi.lib(), n)
        assert getattr(capi.lib(), n).argtypes is not None
    assert "rr_api_levels.h" in capi.LIB_SOURCES
    for m in ("refine_sublist_device", "render_adaptive_levels", "render_adaptive_levels_device"):
        assert hasattr(capi.DeviceScene, m)
    from rustray_amd import renderer
    assert hasattr(renderer, "render_adaptive_levels_torch")
    for m in ("render_adaptive_levels", "render_adaptive_levels_on_device"):
        assert hasattr(renderer.Raytracing, m)
    hpp = open(os.path.join(ROOT, "include", "rustray_host.hpp")).read()
    shim = open(os.path.join(ROOT, "rustray_amd", "csrc", "host_shim.cpp")).read()
    for m in ("render_adaptive_levels", "render_adaptive_levels_device"):
        assert re.search(r"\b" + m + r"\(", hpp) and ("rh_" + m + "(") in shim
    hdr = open(os.path.join(ROOT, "include", "rustray_hip.h")).read()
    assert "#define RR_MAX_ADAPTIVE_LEVELS 8u" in hdr


def test_binding_refuses_what_a_uint16_cannot_hold():
    with pytest.raises(ValueError):
        capi._levels((6, 70000), None)
    with pytest.raises(ValueError):
        capi._levels((6, 14), [None])
    counts, keep, tables = capi._levels((6, 14), [None, np.zeros((14, 2), np.uint16)])
    assert counts.dtype == np.uint16 and list(counts) == [6, 14] and tables is not None and keep[0][0] is None
