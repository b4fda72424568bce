"""albedo=True in the denoising pipelines: one rr_surface_pixels call more on the same stream makes the current camera's albedo and the
filter runs on albedo-demodulated colour.  Python, torch and C++ equal, bit for bit, the yardstick chain render_pixel_parts ->
surface_pixels -> denoise.atrous_denoise(records, halves, albedo); with albedo=False the pipelines return what they return without the
argument.  On a checkered floor the filter with and without the albedo is measured against the truth: the figures are printed, and the
expected direction, which does not hold there, is written down and not asserted (test_quality_on_a_checkered_floor).

One MI355X, floor pixels of the scene below (853 of 50x38), 8 samples in two halves, truth at 512 samples, RMSE of linear colour:
raw 0.042100, filter without albedo 0.085182, filter with albedo 0.218705."""
import ctypes as C

import numpy as np
import pytest

from rustray_amd import renderer
from rustray_amd.denoise import atrous_denoise
from rustray_amd.flat import make_config
from rustray_amd.renderer import Raytracing, TemporalState, _pack_records
from rustray_amd.temporal import AccumulateParams, accumulate_records, previous_view
from tests.helpers import camera_for
from tests.test_cpp_host import _cam_args
from tests.test_gpu_pixel_parts_cpp import _shim

pytestmark = pytest.mark.gpu

W, H = 50, 38
N = W * H
F = np.float32


def _rich():
    from tools.fuzz_parity import rich_scene
    return rich_scene(9119)


def _cfg(samples=8, seed=3):
    return make_config(samples=samples, monte_carlo=True, seed=seed, max_recursion=4)


def _u32(a):
    if hasattr(a, "cpu"):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, F).view(np.uint32)


def test_render_denoised_with_albedo_in_python_torch_and_cpp(hip):
    import torch
    fs = _rich()
    camera = camera_for(fs, W, H)
    rt = Raytracing(fs, camera, 0)
    try:
        rt.config = _cfg()
        base = rt.render_pixel_parts(n_parts=2)
        records, halves = _pack_records(base), _pack_records(base["parts"])
        albedo = rt.albedo()
        surf = rt.surface_pixels()
        assert albedo.shape == (N, 3) and np.array_equal(_u32(albedo), _u32(surf["base_color"][:, :3]))
        hit = surf["hit"] == 1
        assert hit.any() and (~hit).any() and not albedo[~hit].any() and len(np.unique(albedo[hit], axis=0)) > 8     # a textured frame with a background
        want = atrous_denoise(records, halves, albedo, W, H)
        plain = atrous_denoise(records, halves, None, W, H)
        assert not np.array_equal(_u32(want["records"]), _u32(plain["records"]))                                      # the albedo changes the answer
        # Python
        got = rt.render_denoised(albedo=True)
        assert np.array_equal(_u32(got["noisy"]), _u32(records)) and np.array_equal(_u32(got["albedo"]), _u32(albedo))
        differ = int((_u32(got["records"]) != _u32(want["records"])).sum())
        assert differ == 0, differ
        assert np.array_equal(_u32(got["variance"]), _u32(want["variance"]))
        # albedo=False is the call without the argument
        off, default = rt.render_denoised(albedo=False), rt.render_denoised()
        assert "albedo" not in off and np.array_equal(_u32(off["records"]), _u32(default["records"])) and np.array_equal(_u32(off["records"]), _u32(plain["records"]))
        # torch: three calls on one stream, no host trip
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            t = renderer.render_denoised_torch(rt.device_scene, camera.c_struct(), rt.config, albedo=True)
            t_off = renderer.render_denoised_torch(rt.device_scene, camera.c_struct(), rt.config, albedo=False)
            t_default = renderer.render_denoised_torch(rt.device_scene, camera.c_struct(), rt.config)
        st.synchronize()
        assert np.array_equal(_u32(t["records"]), _u32(want["records"])) and np.array_equal(_u32(t["albedo"]), _u32(albedo))
        assert np.array_equal(_u32(t["halves"]), _u32(halves)) and np.array_equal(_u32(t["variance"]), _u32(want["variance"]))
        assert "albedo" not in t_off and np.array_equal(_u32(t_off["records"]), _u32(t_default["records"])) and np.array_equal(_u32(t_off["records"]), _u32(plain["records"]))
    finally:
        rt.device_scene.close()
    # C++: Raytracing::render_denoised(params, rgba8, noisy, with_albedo) and Raytracing::albedo through host_shim.cpp
    L = _shim()
    cam_types = list(L.rh_render_pixel_parts.argtypes[1:10])
    L.rh_render_denoised_albedo.argtypes = [C.c_void_p] + cam_types + [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    fs2 = _rich()
    cs = fs2.c_struct()
    h = L.rh_scene_create(C.byref(cs), 0)
    assert h
    cfg = _cfg()
    args = _cam_args(camera) + (C.byref(cfg), W, H)
    try:
        out, noisy, alb = np.zeros((N, 8), F), np.zeros((N, 8), F), np.ones((N, 3), F)
        assert L.rh_render_denoised_albedo(h, *args, None, 1, out.ctypes.data, noisy.ctypes.data, alb.ctypes.data) == 0
        assert np.array_equal(_u32(noisy), _u32(records)) and np.array_equal(_u32(alb), _u32(albedo))
        assert np.array_equal(_u32(out), _u32(want["records"]))
        assert L.rh_render_denoised_albedo(h, *args, None, 0, out.ctypes.data, None, None) == 0
        assert np.array_equal(_u32(out), _u32(plain["records"]))
    finally:
        L.rh_scene_destroy(h)


def test_render_temporal_with_albedo_over_three_frames(hip):
    import torch
    fs = _rich()
    camera = camera_for(fs, W, H)
    rt = Raytracing(fs, camera, 0)
    try:
        rt.config = _cfg(samples=4)
        albedo = rt.albedo()
        state, state_off, state_default = TemporalState(), TemporalState(), TemporalState()
        hist = dict(records=None, halves=None, length=None)
        view = previous_view(camera)
        for k in range(3):
            got = rt.render_temporal(state, samples=4, seed=100 + k, albedo=True)
            off = rt.render_temporal(state_off, samples=4, seed=100 + k, albedo=False)
            default = rt.render_temporal(state_default, samples=4, seed=100 + k)
            torch.cuda.synchronize()
            rt.config.seed = 100 + k
            base = rt.render_pixel_parts(n_parts=2)
            records, halves = _pack_records(base), _pack_records(base["parts"])
            hist = accumulate_records(records, halves, hist["records"], hist["halves"], hist["length"], None, camera,
                                      AccumulateParams(prev_world_to_clip=view[0], prev_eye=view[1]))
            want = atrous_denoise(hist["records"], hist["halves"], albedo, W, H)
            plain = atrous_denoise(hist["records"], hist["halves"], None, W, H)
            assert np.array_equal(_u32(got["albedo"]), _u32(albedo)), k
            assert np.array_equal(_u32(got["accumulated"]), _u32(hist["records"])), k                 # the accumulation is not changed
            assert np.array_equal(_u32(got["accumulated_halves"]), _u32(hist["halves"])) and np.array_equal(_u32(got["length"]), _u32(hist["length"])), k
            differ = int((_u32(got["records"]) != _u32(want["records"])).sum())
            assert differ == 0, (k, differ)
            assert not np.array_equal(_u32(want["records"]), _u32(plain["records"])), k
            assert "albedo" not in off and np.array_equal(_u32(off["records"]), _u32(default["records"])) and np.array_equal(_u32(off["records"]), _u32(plain["records"])), k
        assert state.frames == 3
    finally:
        rt.device_scene.close()


def _checkered_floor():
    """A floor with a nearest-filter checker as its base texture, one plain sphere over it and one light."""
    from rustray_amd.flat import FlatScene, Item, Light, Material
    from tests import corner_scenes as cs
    fs = FlatScene()
    checker = np.full((16, 16, 4), 255, np.uint8)
    checker[::2, ::2, :3] = 40
    checker[1::2, 1::2, :3] = 40
    fs.textures = [checker]
    fs.meshes = [cs._quad(0.0, 4.0)]
    fm = Material(base_color=(0.9, 0.8, 0.7), ambient_color=(0.1, 0.1, 0.1))
    fm.texture[0] = 0
    fm.texture_filtering_nearest = True
    cs._mesh_item(fs, 0, fm, 3, "floor")
    mi, ci = cs._mat(fs, Material(base_color=(0.2, 0.7, 0.3), ambient_color=(0.05, 0.1, 0.05)))
    t = cs.EYE.copy(); t[:3, 3] = (0.5, 1.0, -0.5); ti = cs.EYE.copy(); ti[:3, 3] = (-0.5, -1.0, 0.5)
    fs.items.append(Item(kind=0, id=6, material=mi, material_cache=ci, radius=1.0, trans=t, trans_inv=ti, bbox_min=(-1.0,) * 3, bbox_max=(1.0,) * 3, name="ball"))
    fs.lights = [Light(pos=(2.0, 7.0, 3.0), intensity=70.0)]
    cs._cam(fs, eye=(0.0, 3.0, 6.0), direction=(0.0, -0.35, -1.0))
    return fs


def test_quality_on_a_checkered_floor(hip):
    """The filter with and without the albedo against the 512-sample truth, over the floor's pixels (default parameters, 8 samples in two
    halves, monte_carlo on): the three RMSEs are printed, split once more into the pixels whose 3x3 neighbourhood shows one checker colour
    and the ones at a colour edge.  THE EXPECTED DIRECTION (with albedo <= without) DOES NOT HOLD on this scene and is not asserted; the
    figures of one MI355X are in DESIGN.md section 8 item 20 with the reason: at 50x38 a checker cell is a few pixels wide, a pixel at a
    cell edge averages both colours over its sub-samples while the albedo is the ONE colour under its centre, and the demodulated value of
    such a pixel (and the ambient term, which the base texture does not modulate) is spread by the filter.  What IS asserted: the two
    pipelines filtered the same noisy frame, both colours of the checker are in view, and every figure is finite."""
    fs = _checkered_floor()
    camera = camera_for(fs, W, H)
    rt = Raytracing(fs, camera, 0)
    try:
        rt.config = _cfg(samples=512)
        truth = rt.render_pixels()["color"].astype(np.float64)
        rt.config = _cfg(samples=8)
        with_albedo = rt.render_denoised(albedo=True)
        without = rt.render_denoised()
        surf = rt.surface_pixels()
    finally:
        rt.device_scene.close()
    floor = (surf["hit"] == 1) & (surf["object_id"] == 3)
    assert floor.sum() > N // 4 and len(np.unique(with_albedo["albedo"][floor], axis=0)) == 2            # both colours of the checker are in view
    assert np.array_equal(_u32(with_albedo["noisy"]), _u32(without["noisy"]))
    a = np.pad(with_albedo["albedo"][:, 0].reshape(H, W), 1, mode="edge")
    near = np.stack([a[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)])
    inside = ((near.max(0) == near.min(0)).reshape(N)) & floor
    edge = floor & ~inside
    rmse = lambda c, at: float(np.sqrt(((c[at].astype(np.float64) - truth[at]) ** 2).mean()))
    figures = {}
    for what, at in (("floor", floor), ("inside a cell", inside), ("at a cell edge", edge)):
        raw, plain, guided = rmse(with_albedo["noisy"][:, 0:3], at), rmse(without["records"][:, 0:3], at), rmse(with_albedo["records"][:, 0:3], at)
        figures[what] = (raw, plain, guided)
        print(f"checkered floor, {what}, {int(at.sum())} pixels, RMSE against 512 samples: raw {raw:.6f}, filter without albedo {plain:.6f}, with albedo {guided:.6f}")
    assert np.isfinite(np.array(list(figures.values()))).all()
