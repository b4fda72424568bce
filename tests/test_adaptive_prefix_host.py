"""Refinement that keeps its samples, without a GPU: the arithmetic the resident-accumulator kernels share with the host
(rustray_amd/csrc/rr_adaptive.h) under AddressSanitizer + UBSan on the CPU, what rr_render_pixel_prefix, rr_render_adaptive_prefix and
their device forms refuse before they touch a device, and the host loop Raytracing.render_adaptive_prefix against a stub scene."""
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

NEW = ("rr_render_pixel_prefix", "rr_render_pixel_prefix_device", "rr_render_adaptive_prefix", "rr_render_adaptive_prefix_device")


def test_prefix_arithmetic_under_asan(tmp_path):
    exe = str(tmp_path / "adaptive_prefix_test")
    cmd = ["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-o", exe, os.path.join(ROOT, "tests", "native", "adaptive_prefix_test.cpp")]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "adaptive prefix test OK" in out.stdout, out.stdout + out.stderr


def test_prefix_refusals_without_a_device():
    """Every call below is refused on its arguments alone, before the scene is looked at: the made-up handle is never dereferenced."""
    L = capi.lib()
    cam = _camera()
    n = 50 * 38
    S = 30
    cfg = make_config(samples=S)
    out = (rr_radiance * n)()
    halves = (rr_radiance * (2 * n))()
    C.memset(out, 0x5a, C.sizeof(out)); C.memset(halves, 0x5a, C.sizeof(halves))
    out_p, halves_p = C.cast(out, C.c_void_p), C.cast(halves, C.c_void_p)
    fake = C.c_void_p(0x1000)

    def host(used=6, o=out_p, hv=None, scene=fake, camera=cam, n_pixels=n):
        return L.rr_render_pixel_prefix(scene, C.byref(camera), C.byref(cfg), None, None, n_pixels, used, o, hv, None, None)

    def device(used=6, o=out_p, hv=None, scene=fake, camera=cam, n_pixels=n, rgba=None):
        return L.rr_render_pixel_prefix_device(scene, C.byref(camera), C.byref(cfg), None, None, n_pixels, used, o, hv, rgba, None, None)

    for call in (host, device):
        assert call(scene=None) == -1
        for used in (0, S + 1):
            assert call(used=used) == -1
            assert b"samples_used" in L.rr_last_error() and str(used).encode() in L.rr_last_error()
        for used in (1, 7, 29):                                       # an odd count is refused with halves only, and the message names the rule
            assert call(used=used, hv=halves_p) == -1
            assert b"halves" in L.rr_last_error() and b"equal" in L.rr_last_error() and b"odd" in L.rr_last_error()
        assert call(o=None) == -1 and b"out" in L.rr_last_error()
        assert call(n_pixels=n - 1) == -1                             # rr_render_pixels' rule: without a list, the whole frame
        assert call(camera=_camera(0, 38)) == -1
    assert device(o=C.c_void_p(C.addressof(out) + 8)) == -1 and b"aligned" in L.rr_last_error()
    assert device(hv=C.c_void_p(C.addressof(halves) + 8)) == -1 and b"halves_out_dev" in L.rr_last_error()
    assert device(rgba=C.c_void_p(C.addressof(out) + 2)) == -1 and b"aligned" in L.rr_last_error()
    assert bytes(out) == b"\x5a" * C.sizeof(out) and bytes(halves) == b"\x5a" * C.sizeof(halves)


def _prefixes(*counts):
    return (C.c_uint16 * max(len(counts), 1))(*counts)


def test_fused_call_refusals_without_a_device():
    L = capi.lib()
    cam = _camera()
    n = 50 * 38
    out = (rr_radiance * n)()
    C.memset(out, 0x5a, C.sizeof(out))
    out_p = C.cast(out, C.c_void_p)
    fake = C.c_void_p(0x1000)
    level_pixels = (C.c_uint32 * 8)(*([77] * 8))

    def host(prefixes=(6, 14, 30), n_levels=None, thr=0.1, o=out_p, camera=cam, scene=fake, samples=30):
        cfg = make_config(samples=samples)
        return L.rr_render_adaptive_prefix(scene, C.byref(camera), C.byref(cfg), None, _prefixes(*prefixes), len(prefixes) if n_levels is None else n_levels, thr, o,
                                           None, None, None, level_pixels, None)

    def device(prefixes=(6, 14, 30), n_levels=None, thr=0.1, o=out_p, camera=cam, scene=fake, samples=30, smp=None, error=None, rgba=None):
        cfg = make_config(samples=samples)
        return L.rr_render_adaptive_prefix_device(scene, C.byref(camera), C.byref(cfg), None, _prefixes(*prefixes), len(prefixes) if n_levels is None else n_levels, thr, o,
                                                  rgba, smp, error, level_pixels, None, None)

    for call in (host, device):
        assert call(scene=None) == -1
        for nl in (0, 1, 9):
            assert call(prefixes=(6, 8, 10, 12, 14, 16, 18, 20, 22), n_levels=nl, samples=22) == -1
            assert b"n_levels" in L.rr_last_error() and str(nl).encode() in L.rr_last_error()
        for prefixes, at in (((7, 14, 30), 0), ((6, 15, 30), 1), ((0, 14, 30), 0)):                         # odd prefixes, a prefix of 0
            assert call(prefixes=prefixes) == -1
            assert b"halves" in L.rr_last_error() and b"equal" in L.rr_last_error() and f"prefix_samples[{at}]".encode() in L.rr_last_error()
        assert call(prefixes=(6, 14, 31), samples=31) == -1 and b"prefix_samples[2]" in L.rr_last_error()   # an odd last prefix, though it is config->samples
        for prefixes, at in (((6, 6, 30), 1), ((6, 14, 14), 2), ((6, 14, 12), 2), ((16, 6, 30), 1)):        # equal or decreasing prefixes
            assert call(prefixes=prefixes) == -1
            assert f"prefix_samples[{at}]".encode() in L.rr_last_error() and b"increase strictly" in L.rr_last_error()
        for samples in (32, 28, 14):                                                                       # the ladder does not end at config->samples
            assert call(samples=samples) == -1
            assert b"prefix_samples[2]" in L.rr_last_error() and b"last prefix" in L.rr_last_error() and str(samples).encode() in L.rr_last_error()
        assert call(prefixes=(6, 14, 16384), samples=16384) == -2 and b"samples" in L.rr_last_error()       # rr_render's rule for the built-in table
        assert call(thr=float("nan")) == -1 and b"NaN" in L.rr_last_error()
        assert call(o=None) == -1 and b"out" in L.rr_last_error()
        assert call(camera=_camera(0, 38)) == -1
        assert call(camera=_camera(32768, 16385)) == -2 and b"2^30" in L.rr_last_error()
    assert device(o=C.c_void_p(C.addressof(out) + 8)) == -1 and b"aligned" in L.rr_last_error()
    assert device(smp=C.c_void_p(C.addressof(out) + 1)) == -1 and b"aligned" in L.rr_last_error()
    assert device(error=C.c_void_p(C.addressof(out) + 2)) == -1 and device(rgba=C.c_void_p(C.addressof(out) + 2)) == -1
    assert bytes(out) == b"\x5a" * C.sizeof(out) and list(level_pixels) == [77] * 8


def test_the_new_entry_points_are_guarded_and_bound():
    src = host_api_source()
    for n in NEW:
        assert re.search(r'^int ' + n + r'\([^{]*\) try \{', src, re.M), f"{n} is not a function-try-block"
        assert f'RR_GUARD_END("{n}")' in src
        assert n in capi.EXPORTS and hasattr(capi.lib(), n)
        assert getattr(capi.lib(), n).argtypes is not None
    assert "rr_api_prefix.h" in capi.LIB_SOURCES
    mk = open(os.path.join(ROOT, "rustray_amd", "csrc", "Makefile")).read()
    assert "rr_api_prefix.h" in mk
    for m in ("render_pixel_prefix", "render_pixel_prefix_device", "render_adaptive_prefix", "render_adaptive_prefix_device"):
        assert hasattr(capi.DeviceScene, m)
    from rustray_amd import renderer
    assert hasattr(renderer, "render_adaptive_prefix_torch")
    for m in ("render_pixel_prefix", "render_adaptive_prefix", "render_adaptive_prefix_on_device"):
        assert hasattr(renderer.Raytracing, m)
    hpp = open(os.path.join(ROOT, "include", "rustray_host.hpp")).read()
    shim = open(os.path.join(ROOT, "rustray_amd", "csrc", "host_shim.cpp")).read()
    for m in ("render_pixel_prefix", "render_adaptive_prefix", "render_adaptive_prefix_device"):
        assert re.search(r"\b" + m + r"\(", hpp) and ("rh_" + m + "(") in shim
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in NEW:
        assert f"pub fn {n}(" in integration


# ---- the host loop against a stub ------------------------------------------------------------------------------------------------
W, H = 21, 13            # partial 8x8 blocks in both directions


def _sample_colour(pixel, s):
    """The colour of sample s of pixel `pixel` (y * W + x) of the stub's frame: noisy pixels (pixel % 3 != 0) have samples that differ,
    and their noise dies out at a sample count that depends on the pixel."""
    calm_from = (pixel % 5) * 6
    noise = 0.0 if (pixel % 3 == 0 or s >= calm_from) else (0.2 if s % 2 == 0 else -0.2)
    return np.float32(0.5 + noise) * np.array([1.0, 0.5, 0.25], np.float32)


class _StubScene:
    """render_pixel_prefix of a made-up frame whose samples are _sample_colour: means over the first samples_used samples and over the two
    interleaved halves, in float32.  It records the calls."""

    def __init__(self):
        self.calls = []

    def render_pixel_prefix(self, cam, cfg, pixels=None, samples_used=1, halves=False, sample_xy=None, rgba8=False, cancel=None):
        assert halves and samples_used % 2 == 0 and sample_xy is None
        if pixels is None:
            idx = np.arange(W * H)
        else:
            xy = np.asarray(pixels, np.uint32)
            idx = (xy >> np.uint32(16)).astype(np.int64) * W + (xy & np.uint32(0xffff)).astype(np.int64)
        self.calls.append((int(cfg.samples), int(samples_used), len(idx)))
        n = len(idx)
        color, parts = np.zeros((n, 3), np.float32), np.zeros((n, 2, 3), np.float32)
        for i, p in enumerate(idx):
            c = np.stack([_sample_colour(int(p), s) for s in range(samples_used)])
            color[i] = c.mean(axis=0, dtype=np.float32)
            parts[i, 0], parts[i, 1] = c[0::2].mean(axis=0, dtype=np.float32), c[1::2].mean(axis=0, dtype=np.float32)
        return dict(color=color, depth=np.full(n, samples_used, np.float32), normal=np.zeros((n, 3), np.float32), object_id=idx.astype(np.uint32),
                    parts=dict(color=parts))


class _StubCamera:
    def c_struct(self):
        return _camera(W, H)


def _stub_rt(samples):
    from rustray_amd.renderer import Raytracing
    rt = object.__new__(Raytracing)
    rt.camera, rt.config, rt.device_scene = _StubCamera(), make_config(samples=samples), _StubScene()
    return rt


@pytest.mark.parametrize("threshold", (0.1, -1.0, 2.0))
def test_host_loop_against_a_plain_per_pixel_loop(threshold):
    prefixes = (6, 14, 30)
    rt = _stub_rt(30)
    got = rt.render_adaptive_prefix(prefixes, threshold)
    # the plain loop: a pixel climbs while its error at the prefix exceeds the threshold
    stub = _StubScene()
    want_samples, want_error, want_color = np.zeros(W * H, np.uint32), np.zeros(W * H, np.float32), np.zeros((W * H, 3), np.float32)
    reached = [0, 0, 0]
    for p in range(W * H):
        xy = np.array([(p % W) | ((p // W) << 16)], np.uint32)
        for l, k in enumerate(prefixes):
            r = stub.render_pixel_prefix(None, rt.config, pixels=xy, samples_used=k, halves=True)
            e = adaptive.half_error(r["parts"]["color"])[0]
            reached[l] += 1
            want_samples[p], want_error[p], want_color[p] = k, e, r["color"][0]
            if not np.float32(e) > np.float32(threshold):
                break
    assert np.array_equal(got["samples"], want_samples) and np.array_equal(got["error"].view(np.uint32), want_error.view(np.uint32))
    assert np.array_equal(got["color"].view(np.uint32), want_color.view(np.uint32))
    assert np.array_equal(got["depth"], want_samples.astype(np.float32)) and np.array_equal(got["object_id"], np.arange(W * H, dtype=np.uint32))
    assert got["level_pixels"] == reached and got["padded"][0] == W * H
    assert got["padded"][1:] == [(c + 63) // 64 * 64 for c in reached[1:]]
    # one call per level reached, every one on the frame of config.samples samples, none of them on an empty list
    assert rt.device_scene.calls == [(30, k, n) for k, n in zip(prefixes, got["padded"]) if n]
    if threshold == 0.1:
        assert W * H > reached[1] > reached[2] > 0
    if threshold < 0:
        assert reached == [W * H] * 3
    if threshold > 1:
        assert reached == [W * H, 0, 0]


def test_host_loop_refuses_a_ladder_that_does_not_end_at_the_frame():
    rt = _stub_rt(32)
    with pytest.raises(ValueError):
        rt.render_adaptive_prefix((6, 14, 30), 0.1)
    assert rt.device_scene.calls == []
