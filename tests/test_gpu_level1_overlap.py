"""Level 1 in stages on two streams (rr_api_frame.h run_level1_stages): k_shade<true> of stage k + 1 beside k_trace_shadow<true> of
stage k, the stages rotating through 2 or 3 shadow-queue buffers.  The schedule may not change one bit of a frame: 152 x 120 at
16 spp = 291 840 primary rays = 5 stages of 65 536 (the last one partial, the buffers wrapped) against the one-stage frame of the
default tuning, which is itself held to the oracle's band; repeated frames on one handle, one enabled light (the buffer stride
equals the stage), RGBA only, the scenes that must keep the serial loop, and two interleaved tile regions."""
import copy

import numpy as np
import pytest

from rustray_amd.flat import make_config
from tests.helpers import assert_in_band, camera_for, compare_frames, load_scene

pytestmark = pytest.mark.gpu

W, H, SPP, CHUNK, STAGES = 152, 120, 16, 65536, 5
KEYS = ("rgba", "normal", "depth", "object_id")
COUNTERS = ("primary_rays", "secondary_rays", "shadow_rays", "shaded_hits")


def _scene(one_light=False, no_lights=False):
    from tools.fuzz_parity import rich_scene   # texture maps of every kind, alpha, several lights (tests/test_gpu_shadow_slots.py)
    fs = rich_scene(9119)
    assert len(fs.items) >= 17 and sum(1 for l in fs.lights if l.enabled) >= 2
    if one_light or no_lights:
        lights, kept = [], no_lights
        for l in fs.lights:
            l = copy.copy(l)
            if l.enabled and kept:
                l.enabled = False
            kept = kept or l.enabled
            lights.append(l)
        fs.lights = lights
        assert sum(1 for l in fs.lights if l.enabled) == (0 if no_lights else 1)
    return fs


def _cfg():
    return make_config(samples=SPP, monte_carlo=True, seed=9119, max_recursion=4)


def _same(a, b, keys=KEYS):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=(a[k].dtype.kind == "f")), k


def _pair(ds, cam, cfg, aux=True):
    """Frame A (default tuning: one stage, serial) and frame B (65 536-ray stages), with their counters and stage counts."""
    ds.set_tuning(shade_chunk_rays=0)
    a = ds.render(cam, cfg, aux=aux); sa, na = ds.stats(), ds.overlap_stages()
    ds.set_tuning(shade_chunk_rays=CHUNK)
    b = ds.render(cam, cfg, aux=aux); sb, nb = ds.stats(), ds.overlap_stages()
    return a, sa, na, b, sb, nb


@pytest.fixture(scope="module")
def rich():
    return _scene()


def test_staged_frame_is_the_serial_frame_and_in_the_oracle_band(hip, oracle, rich):
    assert W * H * SPP == 291840 and -(-W * H * SPP // CHUNK) == STAGES
    cam = camera_for(rich, W, H).c_struct()
    cfg = _cfg()
    with hip.DeviceScene(rich, 0) as ds:
        a, sa, na, b, sb, nb = _pair(ds, cam, cfg)
    assert na == 0 and nb == STAGES
    _same(a, b)
    for k in COUNTERS:
        assert sa[k] == sb[k], k
    assert sa["primary_rays"] == W * H * SPP and sa["shadow_rays"] > 0
    ref = oracle.render(rich.c_struct(), cam, cfg, want_means=True, n_threads=8, want_counters=True)
    res = compare_frames(a, ref)
    assert res["n_rgb_over"] == 0 and res["n_id_diff"] == 0 and res["nan_mismatch"] == 0, res
    assert_in_band(res)
    assert sa["shadow_rays"] <= ref["counters"]["rays_shadow"]


def test_repeated_staged_frames_on_one_handle(hip, rich):
    """Events and buffers are reused from frame to frame: three staged frames back to back, then a serial one, all identical."""
    cam = camera_for(rich, W, H).c_struct()
    cfg = _cfg()
    with hip.DeviceScene(rich, 0) as ds:
        ds.set_tuning(shade_chunk_rays=CHUNK)
        frames = []
        for _ in range(3):
            frames.append(ds.render(cam, cfg))
            assert ds.overlap_stages() == STAGES
        ds.set_tuning(shade_chunk_rays=0)
        a = ds.render(cam, cfg)
        assert ds.overlap_stages() == 0
    for f in frames:
        _same(a, f)


def test_one_enabled_light(hip):
    """The flagship's shape: one enabled light, the stride between buffers equals the stage."""
    fs = _scene(one_light=True)
    cam = camera_for(fs, W, H).c_struct()
    with hip.DeviceScene(fs, 0) as ds:
        a, sa, na, b, sb, nb = _pair(ds, cam, _cfg())
    assert na == 0 and nb == STAGES
    _same(a, b)
    for k in COUNTERS:
        assert sa[k] == sb[k], k
    assert sa["shadow_rays"] > 0


def test_rgba_only(hip, rich):
    cam = camera_for(rich, W, H).c_struct()
    with hip.DeviceScene(rich, 0) as ds:
        a, sa, na, b, sb, nb = _pair(ds, cam, _cfg(), aux=False)
    assert na == 0 and nb == STAGES
    _same(a, b, ("rgba",))


def test_dense_queue_and_unlit_scenes_keep_the_serial_loop(hip):
    """A scene below 17 items (level 1 uses the dense shadow queue) and the rich scene with every light disabled: 65 536-ray chunks, no stages."""
    small = load_scene("spheres")
    assert len(small.items) < 17
    for fs in (small, _scene(no_lights=True)):
        cam = camera_for(fs, W, H).c_struct()
        with hip.DeviceScene(fs, 0) as ds:
            a, sa, na, b, sb, nb = _pair(ds, cam, _cfg())
        assert na == 0 and nb == 0
        _same(a, b)


def test_two_interleaved_tile_regions(hip, rich):
    """Ranks 0 and 1 of a 2-way tiling (32 x 8 tiles) in 65 536-ray stages, stitched together = frame A."""
    import torch
    from rustray_amd.renderer import TiledFrame, region_pixels, render_region_torch
    cam = camera_for(rich, W, H).c_struct()
    cfg = _cfg()
    with hip.DeviceScene(rich, 0) as ds:
        a = ds.render(cam, cfg)
        assert ds.overlap_stages() == 0
        ds.set_tuning(shade_chunk_rays=CHUNK)
        got = {k: np.zeros_like(a[k]).reshape(W * H, -1) for k in KEYS}
        for r in range(2):
            tf = TiledFrame(W, H, r, 2, 32, 8)
            part = render_region_torch(ds, cam, cfg, tf, aux=True)
            torch.cuda.synchronize()
            xy = region_pixels(W, H, 32, 8, 2, r)
            assert ds.overlap_stages() == -(-len(xy) * SPP // CHUNK) >= 2
            for k in KEYS:
                got[k][xy[:, 1] * W + xy[:, 0]] = part[k].cpu().numpy().reshape(len(xy), -1)
    _same(a, {k: got[k].reshape(a[k].shape) for k in KEYS})
