"""The deferred join (rr_api_frame.h join_shadow): the staged level 1 leaves the shadow launches of its last two stages running on the
second and third streams, and level 2 runs beside them -- its closest-hit launch always, its shade and shadow launches where the level's
shadow queue keeps clear of the two buffers in use (three stages in three buffers: the last two use buffers 1 and 2, a 65 536-ray chunk fits
buffer 0, and its shade launch waits for stage 0's shadow launch, which read that buffer, instead).
The kernels are the serial loop's and all that concurrent launches share is an integer atomic, so no bit of a frame may change: every case
compares RGBA8, normal, depth, object id and the ray counters against the SAME handle with the staged schedule switched off
(shade_chunk_rays = 0: one stage, the serial loop, nothing ever pending).  Two batches of two stages each use buffers 0 and 1: there every
shade launch of level 2 waits.
160 x 120 at 8 spp = 153 600 primary rays in 65 536-ray stages = three stages; 22 items (inside the 17 .. 512 window of the fixed shadow
slots): the six two-triangle walls of scenes/spheres_room.npz and sixteen spheres, some mirrors, some glass (alpha 0.3, ior 1.5), two
enabled lights and a disabled one."""
import ctypes as C

import numpy as np
import pytest

from rustray_amd.flat import FlatScene, Item, Light, Material, make_config, rr_frame
from rustray_amd.scene import Scene
from tests.helpers import assert_frames_identical, camera_for, load_scene

pytestmark = pytest.mark.gpu

W, H, SPP, CHUNK, STAGES = 160, 120, 8, 65536, 3
COUNTERS = ("primary_rays", "secondary_rays", "shadow_rays", "shaded_hits")
TWO_BATCHES = 128 * 80000   # queue_budget_bytes: plan_frame cuts the 153 600 primary rays into two batches of 76 800 (two stages each)


def tail_scene(kind="mixed", lights=True):
    """kind: "mixed" = a third of the spheres mirrors and a third glass; "plain" = nothing reflects or refracts; "glass" = every item
    reflects and refracts (each hit spawns two children: level 2 outgrows a small arena)."""
    room = load_scene("spheres_room")
    fs = FlatScene()
    fs.name = f"tail_{kind}"
    fs.meshes = list(room.meshes[:6])

    def add(item, m):
        fs.materials.append(m); fs.materials.append(Scene._cache_of(m))
        item.material, item.material_cache = len(fs.materials) - 2, len(fs.materials) - 1
        fs.items.append(item)

    def material(i, colour):
        m = Material(base_color=colour, shininess=60.0)
        mirror, glass = (kind == "mixed" and i % 3 == 1) or kind == "glass", (kind == "mixed" and i % 3 == 2) or kind == "glass"
        if mirror:
            m.reflectivity = 0.6
        if glass:
            m.alpha, m.refraction_index, m.reflectivity = 0.3, 1.5, max(m.reflectivity, 0.2)
        return m

    for i, it in enumerate(room.items[:6]):   # the walls: opaque, a faint mirror in the mixed scene
        wall = Item(kind=1, id=it.id, material=0, material_cache=0, mesh=i, trans=it.trans.copy(), trans_inv=it.trans_inv.copy(), bbox_min=it.bbox_min,
                    bbox_max=it.bbox_max, name=it.name)
        m = material(0, (0.7, 0.7 - 0.05 * i, 0.6))
        if kind == "mixed" and i % 2 == 0:
            m.reflectivity = 0.3
        add(wall, m)
    eye4 = np.eye(4, dtype=np.float32)
    for i in range(16):   # a 4 x 4 grid of spheres in front of the camera, at staggered depths
        x, y, z, r = -4.5 + 3.0 * (i % 4), -3.0 + 2.0 * (i // 4), -8.0 - 1.5 * ((i * 5) % 4), 0.9 + 0.1 * (i % 3)
        t = eye4.copy(); t[:3, 3] = (x, y, z)
        ti = eye4.copy(); ti[:3, 3] = (-x, -y, -z)
        add(Item(kind=0, id=100 + 3 * i, material=0, material_cache=0, radius=r, trans=t, trans_inv=ti, bbox_min=(-r, -r, -r), bbox_max=(r, r, r), name=f"ball{i}"),
            material(i, (0.2 + 0.05 * i, 0.9 - 0.04 * i, 0.4 + 0.03 * (i % 5))))
    fs.lights = [Light(pos=(-4.0, 5.0, -2.0), intensity=120.0, enabled=lights), Light(pos=(0.0, 0.0, -30.0), intensity=50.0, enabled=False),
                 Light(pos=(5.0, 3.0, -4.0), color=(1.0, 0.8, 0.6), intensity=90.0, enabled=lights)]
    fs.meta = {"camera": dict(room.meta["camera"])}
    assert 17 <= len(fs.items) <= 512 and sum(1 for l in fs.lights if l.enabled) == (2 if lights else 0)
    return fs


def _cfg(max_recursion=4):
    return make_config(samples=SPP, monte_carlo=True, seed=4242, max_recursion=max_recursion)


def _frame(ds, cam, cfg, chunk):
    ds.set_tuning(shade_chunk_rays=chunk)
    out = ds.render(cam, cfg)
    return out, ds.stats(), ds.overlap_stages()


def _pair(ds, cam, cfg, what):
    """The serial frame, then the staged frame of the same handle: identical, with identical counters; -> (serial stats, staged stats, stages)."""
    a, sa, na = _frame(ds, cam, cfg, 0)
    b, sb, nb = _frame(ds, cam, cfg, CHUNK)
    assert na == 0, what
    assert_frames_identical(a, b, what)
    for k in COUNTERS:
        assert sa[k] == sb[k], (what, k)
    assert sa["primary_rays"] == W * H * SPP
    return sa, sb, nb


@pytest.fixture(scope="module")
def mixed():
    return tail_scene()


def test_deeper_levels_behind_a_pending_shadow_stage(hip, mixed):
    """(a) levels 2, 3 and 4 hold rays; with kernel timing on, the launches of the second stream are counted and timed as before."""
    assert W * H * SPP == 153600 and -(-W * H * SPP // CHUNK) == STAGES
    cam = camera_for(mixed, W, H).c_struct()
    with hip.DeviceScene(mixed, 0) as ds:
        ds.set_tuning(kernel_timing=1)
        sa, sb, nb = _pair(ds, cam, _cfg(), "mixed scene")
    assert nb == STAGES and sa["secondary_rays"] > 0 and sa["shadow_rays"] > 0 and sa["sliced_levels"] == sb["sliced_levels"] == 0
    assert sa["launches_trace_closest"] >= 4   # level 1 and at least levels 2, 3 and 4
    assert sb["launches_trace_closest"] == sa["launches_trace_closest"] - 1 + STAGES   # a launch per level; level 1: one per stage
    for k in ("launches_trace_closest_level1", "launches_shade_level1", "launches_trace_shadow_level1"):
        assert sa[k] == 1 and sb[k] == STAGES, k
    assert sb["launches_trace_shadow"] > STAGES and sb["ms_trace_shadow"] > sb["ms_trace_shadow_level1"] > 0.0


def test_level_2_empty_joins_in_front_of_the_resolve(hip):
    """(b) nothing reflects or refracts: level 1 spawns no ray, and the pending stage is joined in front of the resolve."""
    fs = tail_scene("plain")
    cam = camera_for(fs, W, H).c_struct()
    with hip.DeviceScene(fs, 0) as ds:
        sa, sb, nb = _pair(ds, cam, _cfg(), "plain scene")
    assert nb == STAGES and sa["secondary_rays"] == 0 and sa["shadow_rays"] > 0


def test_level_1_that_spawns_nothing(hip, mixed):
    """(c) max_recursion = 0: the level's size is not even read back."""
    cam = camera_for(mixed, W, H).c_struct()
    with hip.DeviceScene(mixed, 0) as ds:
        sa, sb, nb = _pair(ds, cam, _cfg(max_recursion=0), "max_recursion 0")
    assert nb == STAGES and sa["secondary_rays"] == 0 and sa["shadow_rays"] > 0


def test_no_enabled_light(hip):
    """(d) no shadow launch at all: the serial loop with 65 536-ray chunks."""
    fs = tail_scene(lights=False)
    cam = camera_for(fs, W, H).c_struct()
    with hip.DeviceScene(fs, 0) as ds:
        sa, sb, nb = _pair(ds, cam, _cfg(), "no light")
    assert nb == 0 and sa["shadow_rays"] == 0 and sa["secondary_rays"] > 0


def test_two_batches(hip, mixed):
    """(e) the join in front of the next batch's start_batch: two batches of 76 800 primary rays, two stages each."""
    cam = camera_for(mixed, W, H).c_struct()
    with hip.DeviceScene(mixed, 0) as ds:
        ds.set_tuning(queue_budget_bytes=TWO_BATCHES)
        sa, sb, nb = _pair(ds, cam, _cfg(), "two batches")
    assert sa["batches"] == sb["batches"] == 2 and nb == 4 and sa["secondary_rays"] > 0


def test_sliced_level_keeps_the_serial_loop(hip):
    """(f) every item glass: level 2 holds more rays than the arena has room for children, so it is shaded in slices (the serial loop,
    unchanged) behind a staged level 1 of one slice."""
    fs = tail_scene("glass")
    cam = camera_for(fs, W, H).c_struct()
    with hip.DeviceScene(fs, 0) as ds:
        ds.set_tuning(queue_budget_bytes=TWO_BATCHES)
        sa, sb, nb = _pair(ds, cam, _cfg(), "sliced level")
    assert sa["sliced_levels"] > 0 and sb["sliced_levels"] > 0 and nb == 4 and sa["secondary_rays"] > sa["primary_rays"]


def test_cancelled_frames_then_a_clean_frame(hip, mixed):
    """(g) a frame stopped by the cancel flag -- set beforehand, and set from the pass callback between the two batches of a progressive
    frame -- returns RR_ERR_CANCELLED, and the frame after it on the same handle is the serial frame.  Neither cancelled frame has a launch
    pending when it ends (the first stops before its first batch, the second behind the join in front of the pass hook's resolve): a flag set
    while launches are pending is a matter of timing no test can arrange; the way out with launches pending on all three streams is
    tests/test_gpu_launch_order.py's (an injected exception between two stages, and the recorded schedule)."""
    cam = camera_for(mixed, W, H).c_struct()
    cfg = _cfg()
    L = hip.lib()
    with hip.DeviceScene(mixed, 0) as ds:
        ref, _, _ = _frame(ds, cam, cfg, 0)
        ds.set_tuning(shade_chunk_rays=CHUNK)
        out = dict(rgba=np.zeros((H, W, 4), np.uint8), normal=np.zeros((H, W, 3), np.float32), depth=np.zeros((H, W), np.float32), object_id=np.zeros((H, W), np.uint32))
        fr = rr_frame(out["rgba"].ctypes.data, out["normal"].ctypes.data, out["depth"].ctypes.data, out["object_id"].ctypes.data)
        flag = C.c_int(1)
        assert L.rr_render(ds._h, C.byref(cam), C.byref(cfg), None, C.byref(fr), C.byref(flag)) == -6 and b"cancel" in L.rr_last_error()
        flag.value = 0
        passes = []

        def on_pass(user, done, total):   # after the first of two batches: the frame's next look at the flag ends it
            passes.append((int(done), int(total)))
            flag.value = 1
            return 0
        cb = hip.PASS_FN(on_pass)
        assert L.rr_render_progressive(ds._h, C.byref(cam), C.byref(cfg), None, C.byref(fr), 2, cb, None, C.byref(flag)) == -6 and b"cancel" in L.rr_last_error()
        assert passes == [(W * H * SPP // 2, W * H * SPP)]
        flag.value = 0
        assert L.rr_render(ds._h, C.byref(cam), C.byref(cfg), None, C.byref(fr), C.byref(flag)) == 0
        assert ds.overlap_stages() == STAGES
    assert_frames_identical(ref, out, "after two cancelled frames")


def test_five_staged_frames_in_a_row(hip, mixed):
    """(h) a missing join shows as a frame that differs from run to run: five staged frames on one handle, each the serial frame."""
    cam = camera_for(mixed, W, H).c_struct()
    cfg = _cfg()
    with hip.DeviceScene(mixed, 0) as ds:
        ref, _, _ = _frame(ds, cam, cfg, 0)
        ds.set_tuning(shade_chunk_rays=CHUNK)
        frames = []
        for _ in range(5):
            frames.append(ds.render(cam, cfg))
            assert ds.overlap_stages() == STAGES
    for i, f in enumerate(frames):
        assert_frames_identical(ref, f, f"staged frame {i}")
