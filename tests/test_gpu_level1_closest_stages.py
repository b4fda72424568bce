"""Level 1 in stages on three streams (rr_api_frame.h run_level1_stages): where the stages cover the whole level, its closest hits are
traced stage by stage too -- k_trace_closest<true> over the packet range of stage k on the handle's third stream, ahead of the shade
launch of stage k.  A ray and its hit record depend on the ray's index alone, so the schedule may not change one bit: every staged
frame (65 536-ray stages) is compared with the one-stage frame of the default tuning by np.array_equal on every buffer, and the four
ray counters are equal.  Cases: a partial last stage, a level whose last packet is partial, packets of one pixel with a sample-group
boundary inside a range, two batches (hit1 rewritten behind the previous batch's last shade launch), repeated frames on one handle,
a cancelled call, RGBA only, kernel timing on and off."""
import ctypes as C

import numpy as np
import pytest

from rustray_amd.flat import make_config, rr_frame
from tests.helpers import camera_for

pytestmark = pytest.mark.gpu

W, H, SPP, CHUNK, STAGES = 152, 120, 16, 65536, 5
KEYS = ("rgba", "normal", "depth", "object_id")
COUNTERS = ("primary_rays", "secondary_rays", "shadow_rays", "shaded_hits")


def _cfg(spp=SPP):
    return make_config(samples=spp, monte_carlo=True, seed=9119, max_recursion=4)


def _same(a, b, keys=KEYS):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=(a[k].dtype.kind == "f")), k


def _render(ds, cam, cfg, chunk, aux=True):
    """One frame with shade_chunk_rays = chunk (0: the default tuning, one stage) -> (frame, stats, overlap stages)."""
    ds.set_tuning(shade_chunk_rays=chunk)
    out = ds.render(cam, cfg, aux=aux)
    return out, ds.stats(), ds.overlap_stages()


def _check_pair(serial, staged, n_stages, keys=KEYS):
    (a, sa, na), (b, sb, nb) = serial, staged
    assert na == 0 and nb == n_stages
    _same(a, b, keys)
    for k in COUNTERS:
        assert sa[k] == sb[k], k


@pytest.fixture(scope="module")
def rich():
    from tools.fuzz_parity import rich_scene   # as tests/test_gpu_level1_overlap.py builds it
    fs = rich_scene(9119)
    assert 17 <= len(fs.items) <= 512 and 2 <= sum(1 for l in fs.lights if l.enabled) <= 32
    return fs


@pytest.fixture(scope="module")
def cam(rich):
    return camera_for(rich, W, H).c_struct()


@pytest.fixture(scope="module")
def serial(hip, rich, cam):
    """The one-stage frame of 152 x 120 at 16 spp, kernel timing on: (frame, stats, overlap stages).  Computed once, never written."""
    with hip.DeviceScene(rich, 0) as ds:
        ds.set_profiling(True)
        got = _render(ds, cam, _cfg(), 0)
    for v in got[0].values():
        v.setflags(write=False)
    return got


def test_five_stages_the_last_partial(hip, rich, cam, serial):
    assert W * H * SPP == 291840 and -(-W * H * SPP // CHUNK) == STAGES and W * H * SPP % CHUNK != 0
    with hip.DeviceScene(rich, 0) as ds:
        ds.set_profiling(True)
        staged = _render(ds, cam, _cfg(), CHUNK)
    _check_pair(serial, staged, STAGES)
    sa, sb = serial[1], staged[1]
    assert sa["primary_rays"] == W * H * SPP and sa["shadow_rays"] > 0
    assert sa["launches_trace_closest_level1"] == 1 and sb["launches_trace_closest_level1"] == STAGES
    assert sb["launches_shade_level1"] == STAGES and sb["launches_trace_shadow_level1"] == STAGES
    assert sa["batches"] == 1 and sb["batches"] == 1
    # the deeper levels keep their one launch per level
    assert sb["launches_trace_closest"] - STAGES == sa["launches_trace_closest"] - 1


def test_partial_last_packet_lies_in_the_last_range(hip, rich):
    w, h = 151, 119
    assert w * h * SPP == 287504 and w * h * SPP % 64 == 16 and -(-w * h * SPP // CHUNK) == 5
    c = camera_for(rich, w, h).c_struct()
    with hip.DeviceScene(rich, 0) as ds:
        a = _render(ds, c, _cfg(), 0)
        b = _render(ds, c, _cfg(), CHUNK)
    _check_pair(a, b, 5)
    assert a[1]["primary_rays"] == w * h * SPP


def test_one_pixel_packets_and_a_group_boundary_inside_a_range(hip, rich):
    w, h, spp = 48, 40, 128
    n = w * h * spp
    assert n == 245760 and -(-n // CHUNK) == 4 and CHUNK < w * h * 64 == 122880 < 2 * CHUNK
    c = camera_for(rich, w, h).c_struct()
    with hip.DeviceScene(rich, 0) as ds:
        ds.set_tuning(sample_group=64)
        a = _render(ds, c, _cfg(spp), 0)
        b = _render(ds, c, _cfg(spp), CHUNK)
    _check_pair(a, b, 4)
    assert a[1]["primary_rays"] == n and a[1]["batches"] == 1 and b[1]["batches"] == 1


def test_two_batches(hip, rich, cam, serial):
    """150 000 primary rays fit the budget (128 B each): two batches of 8 sample slices = 145 920 rays = 3 stages each."""
    with hip.DeviceScene(rich, 0) as ds:
        ds.set_profiling(True)
        ds.set_tuning(queue_budget_bytes=150000 * 128)
        a = _render(ds, cam, _cfg(), 0)
        b = _render(ds, cam, _cfg(), CHUNK)
    assert a[1]["batches"] == 2 and b[1]["batches"] == 2 and a[1]["sliced_levels"] == 0 and b[1]["sliced_levels"] == 0
    _check_pair(a, b, 6)
    assert a[1]["launches_trace_closest_level1"] == 2 and b[1]["launches_trace_closest_level1"] == 6
    _same(serial[0], b[0])   # and the batches change nothing either
    for k in COUNTERS:
        assert serial[1][k] == b[1][k], k


def test_repeated_frames_on_one_handle(hip, rich, cam, serial):
    """The stream and its events are reused: three staged frames back to back, then a serial one."""
    with hip.DeviceScene(rich, 0) as ds:
        for _ in range(3):
            _check_pair(serial, _render(ds, cam, _cfg(), CHUNK), STAGES)
        a = _render(ds, cam, _cfg(), 0)
    assert a[2] == 0
    _same(serial[0], a[0])


def test_cancel_flag_set_before_the_call(hip, rich, cam, serial):
    cfg = _cfg()
    with hip.DeviceScene(rich, 0) as ds:
        ds.set_tuning(shade_chunk_rays=CHUNK)
        rgba = np.zeros((H, W, 4), np.uint8)
        fr = rr_frame(rgba.ctypes.data, None, None, None)
        flag = C.c_int(1)
        rc = hip.lib().rr_render(ds._h, C.byref(cam), C.byref(cfg), None, C.byref(fr), C.byref(flag))
        assert rc == -6 and b"cancel" in hip.lib().rr_last_error()   # RR_ERR_CANCELLED
        _check_pair(serial, _render(ds, cam, cfg, CHUNK), STAGES)


def test_rgba_only(hip, rich, cam, serial):
    with hip.DeviceScene(rich, 0) as ds:
        a = _render(ds, cam, _cfg(), 0, aux=False)
        b = _render(ds, cam, _cfg(), CHUNK, aux=False)
    _check_pair(a, b, STAGES, ("rgba",))
    _same(serial[0], b[0], ("rgba",))


def test_kernel_timing_on_and_off(hip, rich, cam, serial):
    with hip.DeviceScene(rich, 0) as ds:
        ds.set_profiling(True)
        on = _render(ds, cam, _cfg(), CHUNK)
        ds.set_profiling(False)
        off = _render(ds, cam, _cfg(), CHUNK)
    _check_pair(serial, on, STAGES)
    _check_pair(serial, off, STAGES)
    assert on[1]["launches_trace_closest_level1"] == STAGES and off[1]["launches_trace_closest_level1"] == 0
