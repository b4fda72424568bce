"""What k_shade reads through the scalar cache at its point of use.  The kernel keeps in SGPRs only what every packet needs (the hit
records, the chunk bounds, the shadow queue); the planes, the next level's queue, the validity words, the counters, the batch's primary
constants and the slot table are read from its kernel-argument segment where they are used (rr_kernels.hip ShadeArgs), and the record of
light `li` arrives as three 16-byte groups through the constant address space (light_uniform).  Nothing may change by a bit: every launch
shape of the kernel gives one frame, every light kind and the skip of a disabled light match the oracle, the record after the flush of
the lane sums is the right one, a light edit is seen by the next frame, and a frame cut into chunks, stages and tile regions is the frame.

Frames are 32 x 16 at 64 samples with monte_carlo, in the manner of tests/test_gpu_receiver_uniform.py."""
import numpy as np
import pytest

from rustray_amd.flat import FlatScene, Light, Material
from tests.helpers import assert_frames_identical, camera_for
from tests.packet_pad import in_packet_range, pad_inert
from tests.test_gpu_packet_walk import _ball, _camera, _floor, lights_scene
from tests.test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu
COUNTS = ("primary_rays", "secondary_rays", "shaded_hits", "shadow_rays")
W, H = 32, 16
GROUPS = (64, 4, 1)


def _cfg(samples=64, max_recursion=3):
    from rustray_amd.flat import make_config
    return make_config(samples=samples, monte_carlo=True, seed=5, max_recursion=max_recursion)


def _frame(ds, fs, w=W, h=H, cfg=None):
    out = ds.render(camera_for(fs, w, h).c_struct(), cfg or _cfg())
    st = ds.stats()
    return out, [st[k] for k in COUNTS]


def _render(hip, fs, group=64, w=W, h=H, cfg=None):
    with hip.DeviceScene(fs, 0) as ds:
        ds.set_tuning(sample_group=group)
        return _frame(ds, fs, w, h, cfg)


def _same(a, b, what):
    assert_frames_identical(a[0], b[0], what)
    assert a[1] == b[1], (what, a[1], b[1])


def _oracle(oracle, fs, w=W, h=H, cfg=None):
    return oracle.render(fs.c_struct(), camera_for(fs, w, h).c_struct(), cfg or _cfg(), want_means=True, n_threads=16)


def _clone(fs):
    return pad_inert(fs, len(fs.items), "copies")


def _padded(fs, n):
    return fs if n == len(fs.items) else pad_inert(fs, n, "scattered", seed=n)


# ---------------------------------------------------------------------------------------------------------------------------
# every launch shape of k_shade
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shapes(hip):
    """lights_scene at 7 items (dense shadow queue), 17 and 65 (fixed slots, staged launches), each at sample_group 64, 4 and 1: rendered once."""
    base = lights_scene()
    assert len(base.items) == 7 and not in_packet_range(7) and in_packet_range(17) and in_packet_range(65)
    frames = {(n, g): _render(hip, _padded(base, n), g) for n in (7, 17, 65) for g in GROUPS}
    for out, _ in frames.values():
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return base, frames


def test_every_launch_shape_gives_one_frame(shapes):
    """One frame is the reference (7 items, sample_group 64); all nine are identical to it in the four buffers and the four ray counts."""
    _, frames = shapes
    ref = frames[7, 64]
    assert ref[1][3] > 0 and (ref[0]["object_id"] == 0).any() and (ref[0]["object_id"] != 0).any()
    for (n, g), f in frames.items():
        _same(f, ref, f"{n} items, sample_group {g}")


def test_dense_queue_frame_matches_the_oracle(shapes, oracle):
    base, frames = shapes
    assert_parity(frames[7, 64][0], _oracle(oracle, base), "7 items")


# ---------------------------------------------------------------------------------------------------------------------------
# every light kind and the skip
# ---------------------------------------------------------------------------------------------------------------------------
def kinds_scene(receive_shadow):
    """A floor and three balls under a point, a DISABLED, a directional and a spot light.  The disabled light keeps its index: the jitter
    streams of the lights behind it are 1 + their index in the list, not their ordinal among the enabled ones."""
    fs = FlatScene()
    _floor(fs, 2, 0.0, 20.0, Material(base_color=(0.8, 0.8, 0.8), shadow_softness=0.05, receive_shadow=receive_shadow))
    for k, (x, z, r) in enumerate(((-1.5, -3.0, 0.6), (1.2, -4.5, 0.8), (0.0, -1.0, 0.3))):
        _ball(fs, 10 + k, (x, r, z), r, Material(base_color=(0.9 - 0.2 * k, 0.5, 0.3 + 0.2 * k), shininess=30.0, shadow_softness=0.1, receive_shadow=receive_shadow))
    fs.lights = [Light(pos=(0.5, 3.0, -2.0), intensity=60.0, color=(1.0, 0.8, 0.6)),
                 Light(pos=(-2.0, 5.0, 1.0), intensity=500.0, color=(0.0, 1.0, 0.0), enabled=False),
                 Light(dir=(0.3, -1.0, -0.4), intensity=0.4, light_type=0, color=(0.6, 0.7, 1.0)),
                 Light(pos=(-3.0, 5.0, 1.0), dir=(0.4, -1.0, -0.7), intensity=200.0, light_type=2, max_angle=0.5, color=(1.0, 1.0, 0.7))]
    _camera(fs, (0.0, 2.5, 4.0), (0.0, -0.35, -1.0))
    return fs


@pytest.mark.parametrize("receive_shadow", (True, False))
def test_every_light_kind_and_the_skip(hip, oracle, receive_shadow):
    fs = kinds_scene(receive_shadow)
    ref = _oracle(oracle, fs)
    lit = _clone(fs)
    lit.lights[1].enabled = True
    assert not np.array_equal(_oracle(oracle, lit)["rgba"], ref["rgba"])    # the disabled light would be seen
    small = _render(hip, fs)
    assert (small[1][3] > 0) == receive_shadow
    assert_parity(small[0], ref, "4 items")
    for g in (64, 1):
        f = _render(hip, _padded(fs, 17), g)
        assert_parity(f[0], ref, f"17 items, sample_group {g}")
        _same(f, small, f"17 items, sample_group {g}, against 4 items")


# ---------------------------------------------------------------------------------------------------------------------------
# the flush every 32 enabled lights
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_enabled", (33, 65))
def test_light_records_across_the_flush(hip, oracle, n_enabled):
    """33 and 65 enabled lights of all three kinds, each with its own place and colour, on receivers WITHOUT receive_shadow (every term is
    added in k_shade, whose lane sums are flushed after the enabled lights 31 and 63), and a disabled light at index 31: the light at
    index 32 is enabled light 31, and the records behind the flush must be their own."""
    fs = kinds_scene(False)
    rng = np.random.default_rng(n_enabled)
    lights = []
    for i in range(n_enabled + 1):
        kind = i % 3
        lights.append(Light(pos=tuple(float(v) for v in rng.uniform((-4.0, 2.0, -6.0), (4.0, 6.0, 2.0))),
                            dir=(float(rng.uniform(-0.5, 0.5)), -1.0, float(rng.uniform(-0.8, 0.2))), light_type=kind, max_angle=0.9,
                            intensity=(0.02 if kind == 0 else 4.0), color=tuple(float(v) for v in rng.uniform(0.1, 1.0, 3)), enabled=(i != 31)))
    fs.lights = lights
    assert sum(l.enabled for l in fs.lights) == n_enabled
    ref = _oracle(oracle, fs)
    assert 20 < ref["rgba"][..., :3].mean() < 235                           # neither black nor saturated: a wrong record shows
    for n in (len(fs.items), 17):
        out, counts = _render(hip, _padded(fs, n))
        assert counts[3] == 0
        assert_parity(out, ref, f"{n_enabled} lights, {n} items")


# ---------------------------------------------------------------------------------------------------------------------------
# deeper levels
# ---------------------------------------------------------------------------------------------------------------------------
def test_deeper_levels_with_several_lights(hip, oracle):
    """A reflective floor at max_recursion 3: k_shade<false> shades the children under all the lights of kinds_scene."""
    fs = kinds_scene(True)
    for idx in (fs.items[0].material, fs.items[0].material_cache):
        fs.materials[idx].reflectivity = 0.5
    ref = _oracle(oracle, fs)
    frames = {g: _render(hip, _padded(fs, 17), g) for g in GROUPS}
    assert frames[64][1][1] > 0                                            # secondary rays
    assert_parity(frames[64][0], ref, "reflective floor")
    for g in (4, 1):
        _same(frames[g], frames[64], f"sample_group {g} against 64")
    _same(_render(hip, fs), frames[64], "4 items against 17")


# ---------------------------------------------------------------------------------------------------------------------------
# a live light edit
# ---------------------------------------------------------------------------------------------------------------------------
def test_a_light_edit_is_seen_by_the_next_frame(hip):
    """Position, colour and enable flag of lights edited between two frames on one handle: the second frame is that of a fresh scene
    built with the edited lights, at the same number of lights (the records are overwritten in place: the scalar cache must not
    serve the old ones)."""
    fs = _padded(kinds_scene(True), 17)
    edited = _clone(fs)
    edited.lights[0].pos = (-1.0, 2.0, -1.0)
    edited.lights[2].color = (1.0, 0.3, 0.2)
    edited.lights[1].enabled = True
    edited.lights[3].enabled = False
    fresh_before, fresh_after = _render(hip, fs), _render(hip, edited)
    assert not np.array_equal(fresh_before[0]["rgba"], fresh_after[0]["rgba"])
    with hip.DeviceScene(fs, 0) as ds:
        _same(_frame(ds, fs), fresh_before, "before the edit")
        ds.update_lights(edited.lights)
        _same(_frame(ds, edited), fresh_after, "after the edit")
        ds.update_lights(fs.lights)
        _same(_frame(ds, fs), fresh_before, "edited back")


# ---------------------------------------------------------------------------------------------------------------------------
# chunks, stages and tile regions
# ---------------------------------------------------------------------------------------------------------------------------
def test_a_partial_last_packet_and_tile_regions(hip):
    """29 x 16 at 17 items: with sample_group 1 a packet is 64 pixels of one sample and the 464 pixels end inside the eighth packet
    (sample_group 64: whole packets, the same frame).  The frame equals the same frame rendered as the two tile regions of two ranks
    (32 x 8 tiles: one tile each, 232 pixels, a partial packet in both), so chunk_begin, sq_cap and the validity words' row length
    arrive right whatever the launch covers."""
    import torch
    from rustray_amd.renderer import TiledFrame, render_region_torch
    w, h, world = 29, 16, 2
    fs = _padded(lights_scene(), 17)
    cam, cfg = camera_for(fs, w, h).c_struct(), _cfg()
    wholes = {}
    with hip.DeviceScene(fs, 0) as ds:
        for group in (64, 1):
            ds.set_tuning(sample_group=group)
            whole = wholes[group] = ds.render(cam, cfg)
            assert ds.stats()["shadow_rays"] > 0
            parts = [render_region_torch(ds, cam, cfg, TiledFrame(w, h, r, world, 32, 8), aux=True) for r in range(world)]
            torch.cuda.synchronize()
            for key, eb in (("rgba", 4), ("normal", 12), ("depth", 4), ("object_id", 4)):
                cat = torch.cat([p[key].reshape(p[key].shape[0], -1) for p in parts], dim=0).contiguous()
                frame = torch.empty((h * w, cat.shape[1]), dtype=cat.dtype, device=cat.device)
                hip.deinterleave_device(w, h, 32, 8, world, eb, cat.data_ptr(), frame.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                got = frame.cpu().numpy().reshape(whole[key].shape)
                assert np.array_equal(got.view(np.uint8), whole[key].view(np.uint8)), (key, group)
    assert_frames_identical(wholes[1], wholes[64], "sample_group 1 against 64")
