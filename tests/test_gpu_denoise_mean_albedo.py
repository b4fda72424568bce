"""albedo="mean" in the denoising pipelines: one rr_albedo_pixels call with the frame's config and table stands where albedo=True has its
rr_surface_pixels call.  Python, torch and C++ equal, bit for bit, the yardstick chain render_pixel_parts -> albedo_pixels ->
denoise.atrous_denoise(records, halves, mean albedo), over one frame and over three temporal frames; albedo=True and albedo=False return
the bits of the chains of tests/test_gpu_denoise_albedo.py.  On the checkered floor the four arms -- raw, filter without albedo, with the
pixel-centre albedo, with the mean albedo -- are measured against the 512-sample truth (test_quality_on_a_checkered_floor); the figures
of one MI355X are in DESIGN.md section 8 item 21.

One MI355X, RMSE of linear colour, raw / filter without albedo / with the pixel-centre albedo / with the mean albedo:
the floor (853 pixels) 0.042100 / 0.085182 / 0.218705 / 0.106973; inside a cell (64) 0.000203 / 0.094109 / 0.068753 / 0.071278;
at a cell edge (789) 0.043774 / 0.084417 / 0.226557 / 0.109359."""
import ctypes as C

import numpy as np
import pytest

from rustray_amd import renderer
from rustray_amd.denoise import atrous_denoise
from rustray_amd.renderer import Raytracing, TemporalState, _pack_records
from rustray_amd.temporal import AccumulateParams, accumulate_records, previous_view
from tests.helpers import camera_for
from tests.test_cpp_host import _cam_args
from tests.test_gpu_denoise_albedo import F, H, N, W, _cfg, _checkered_floor, _rich, _u32
from tests.test_gpu_pixel_parts_cpp import _shim

pytestmark = pytest.mark.gpu


def test_render_denoised_with_the_mean_albedo_in_python_torch_and_cpp(hip):
    import torch
    fs = _rich()
    camera = camera_for(fs, W, H)
    rt = Raytracing(fs, camera, 0)
    try:
        rt.config = _cfg()
        base = rt.render_pixel_parts(n_parts=2)
        records, halves = _pack_records(base), _pack_records(base["parts"])
        mean = rt.device_scene.albedo_pixels(camera.c_struct(), rt.config)
        centre = rt.albedo()
        assert mean.shape == (N, 3) and np.array_equal(_u32(rt.mean_albedo()), _u32(mean))
        assert not np.array_equal(_u32(mean), _u32(centre))                                       # silhouettes and texture edges mix
        want = atrous_denoise(records, halves, mean, W, H)
        want_centre = atrous_denoise(records, halves, centre, W, H)
        plain = atrous_denoise(records, halves, None, W, H)
        assert not np.array_equal(_u32(want["records"]), _u32(want_centre["records"]))
        # Python
        got = rt.render_denoised(albedo="mean")
        assert np.array_equal(_u32(got["noisy"]), _u32(records)) and np.array_equal(_u32(got["albedo"]), _u32(mean))
        differ = int((_u32(got["records"]) != _u32(want["records"])).sum())
        assert differ == 0, differ
        assert np.array_equal(_u32(got["variance"]), _u32(want["variance"]))
        # True and False return what they returned before "mean" existed
        on, off, default = rt.render_denoised(albedo=True), rt.render_denoised(albedo=False), rt.render_denoised()
        assert np.array_equal(_u32(on["records"]), _u32(want_centre["records"])) and np.array_equal(_u32(on["albedo"]), _u32(centre))
        assert "albedo" not in off and np.array_equal(_u32(off["records"]), _u32(default["records"])) and np.array_equal(_u32(off["records"]), _u32(plain["records"]))
        with pytest.raises(ValueError):
            rt.render_denoised(albedo="centre")
        # torch: three calls on one stream, no host trip
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            t = renderer.render_denoised_torch(rt.device_scene, camera.c_struct(), rt.config, albedo="mean")
            t_on = renderer.render_denoised_torch(rt.device_scene, camera.c_struct(), rt.config, albedo=True)
            t_off = renderer.render_denoised_torch(rt.device_scene, camera.c_struct(), rt.config, albedo=False)
            t_mean = rt.mean_albedo_torch()
        st.synchronize()
        assert np.array_equal(_u32(t["records"]), _u32(want["records"])) and np.array_equal(_u32(t["albedo"]), _u32(mean))
        assert np.array_equal(_u32(t["halves"]), _u32(halves)) and np.array_equal(_u32(t["variance"]), _u32(want["variance"]))
        assert np.array_equal(_u32(t_on["records"]), _u32(want_centre["records"]))
        assert "albedo" not in t_off and np.array_equal(_u32(t_off["records"]), _u32(plain["records"]))
        assert t_mean.is_cuda and np.array_equal(_u32(t_mean), _u32(mean))
    finally:
        rt.device_scene.close()
    # C++: Raytracing::render_denoised(AlbedoGuide::MEAN, ...) and Raytracing::mean_albedo through host_shim.cpp
    L = _shim()
    cam_types = list(L.rh_render_pixel_parts.argtypes[1:10])
    L.rh_render_denoised_mean_albedo.argtypes = [C.c_void_p] + cam_types + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rh_render_denoised_albedo.argtypes = [C.c_void_p] + cam_types + [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    fs2 = _rich()
    cs = fs2.c_struct()
    h = L.rh_scene_create(C.byref(cs), 0)
    assert h
    cfg = _cfg()
    args = _cam_args(camera) + (C.byref(cfg), W, H)
    try:
        out, noisy, alb = np.zeros((N, 8), F), np.zeros((N, 8), F), np.ones((N, 3), F)
        assert L.rh_render_denoised_mean_albedo(h, *args, None, out.ctypes.data, noisy.ctypes.data, alb.ctypes.data) == 0
        assert np.array_equal(_u32(noisy), _u32(records)) and np.array_equal(_u32(alb), _u32(mean))
        assert np.array_equal(_u32(out), _u32(want["records"]))
        assert L.rh_render_denoised_albedo(h, *args, None, 1, out.ctypes.data, None, None) == 0     # with_albedo keeps its bits
        assert np.array_equal(_u32(out), _u32(want_centre["records"]))
        assert L.rh_render_denoised_albedo(h, *args, None, 0, out.ctypes.data, None, None) == 0
        assert np.array_equal(_u32(out), _u32(plain["records"]))
    finally:
        L.rh_scene_destroy(h)


def test_render_temporal_with_the_mean_albedo_over_three_frames(hip):
    import torch
    fs = _rich()
    camera = camera_for(fs, W, H)
    rt = Raytracing(fs, camera, 0)
    try:
        rt.config = _cfg(samples=4)
        mean = rt.mean_albedo()                  # (the albedo does not depend on the seed: one array serves the three frames)
        centre = rt.albedo()
        state, state_on, state_off = TemporalState(), TemporalState(), TemporalState()
        hist = dict(records=None, halves=None, length=None)
        view = previous_view(camera)
        for k in range(3):
            got = rt.render_temporal(state, samples=4, seed=100 + k, albedo="mean")
            on = rt.render_temporal(state_on, samples=4, seed=100 + k, albedo=True)
            off = rt.render_temporal(state_off, samples=4, seed=100 + k, albedo=False)
            torch.cuda.synchronize()
            rt.config.seed = 100 + k
            base = rt.render_pixel_parts(n_parts=2)
            records, halves = _pack_records(base), _pack_records(base["parts"])
            hist = accumulate_records(records, halves, hist["records"], hist["halves"], hist["length"], None, camera,
                                      AccumulateParams(prev_world_to_clip=view[0], prev_eye=view[1]))
            want = atrous_denoise(hist["records"], hist["halves"], mean, W, H)
            want_centre = atrous_denoise(hist["records"], hist["halves"], centre, W, H)
            plain = atrous_denoise(hist["records"], hist["halves"], None, W, H)
            assert np.array_equal(_u32(got["albedo"]), _u32(mean)), k
            assert np.array_equal(_u32(got["accumulated"]), _u32(hist["records"])), k                 # the accumulation is not changed
            differ = int((_u32(got["records"]) != _u32(want["records"])).sum())
            assert differ == 0, (k, differ)
            assert np.array_equal(_u32(on["records"]), _u32(want_centre["records"])) and np.array_equal(_u32(on["albedo"]), _u32(centre)), k
            assert "albedo" not in off and np.array_equal(_u32(off["records"]), _u32(plain["records"])), k
        assert state.frames == 3
    finally:
        rt.device_scene.close()


def test_quality_on_a_checkered_floor(hip):
    """The four arms against the 512-sample truth over the floor's pixels (default parameters, 8 samples in two halves, monte_carlo on),
    split into the pixels whose 3x3 neighbourhood shows one checker colour under the pixels' centres and the ones at a colour edge; every
    figure is printed.  Asserted because it follows from the construction: every floor pixel's mean albedo lies per channel within the two
    checker albedos (a mean of terms that are one or the other; 2^-24 of slack for the rounding of the terms) -- below the lighter one
    everywhere, above the darker one wherever no sub-sample can pass the floor's far edge, where a miss adds 0 --, some edge pixel lies
    strictly between them, all figures are finite, all arms filtered the same noisy frame.  Asserted as the purpose of the feature: at the
    cell-edge pixels the mean-albedo arm's RMSE is below the pixel-centre arm's.  Whether the mean-albedo arm beats the filter without
    albedo is not asserted either way (the ambient term is still divided by the albedo)."""
    fs = _checkered_floor()
    camera = camera_for(fs, W, H)
    rt = Raytracing(fs, camera, 0)
    try:
        rt.config = _cfg(samples=512)
        truth = rt.render_pixels()["color"].astype(np.float64)
        rt.config = _cfg(samples=8)
        with_mean = rt.render_denoised(albedo="mean")
        with_centre = rt.render_denoised(albedo=True)
        without = rt.render_denoised()
        surf = rt.surface_pixels()
    finally:
        rt.device_scene.close()
    floor = (surf["hit"] == 1) & (surf["object_id"] == 3)
    centre, mean = with_centre["albedo"], with_mean["albedo"]
    colours = np.unique(centre[floor], axis=0)
    assert floor.sum() > N // 4 and len(colours) == 2                                                  # both colours of the checker are in view
    lo, hi = colours.min(axis=0), colours.max(axis=0)
    assert np.array_equal(_u32(with_mean["noisy"]), _u32(without["noisy"])) and np.array_equal(_u32(with_centre["noisy"]), _u32(without["noisy"]))
    a = np.pad(centre[:, 0].reshape(H, W), 1, mode="edge")
    near = np.stack([a[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)])
    inside = ((near.max(0) == near.min(0)).reshape(N)) & floor
    edge = floor & ~inside
    # Every term of a floor pixel is one of the two checker albedos, the ball's (0.2, 0.7, 0.3: per channel within them) or a miss (0, where
    # a sub-sample passes the quad's far edge).  So every floor pixel is bounded above by the lighter albedo, and below by the darker one
    # wherever no sub-sample can miss: where the 3x3 neighbourhood of pixel centres is all floor or ball (a sub-sample lies within the pixel).
    solid = np.pad((surf["hit"] == 1).reshape(H, W), 1, mode="constant")
    no_miss = np.stack([solid[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)]).all(0).reshape(N) & floor
    slack = 2.0 ** -24
    low = (mean < lo - slack).any(axis=1) & floor
    print(f"checkered floor: {int(floor.sum())} floor pixels, {int(no_miss.sum())} of them with no miss near; {int(low.sum())} floor pixels below the darker albedo "
          f"(all at the floor's far edge: {bool((low & ~no_miss).sum() == low.sum())})")
    assert no_miss.sum() > floor.sum() * 3 // 4
    assert (mean[floor] <= hi + slack).all() and (mean[floor] >= 0.0).all() and (mean[no_miss] >= lo - slack).all()
    strictly = ((mean > lo + slack) & (mean < hi - slack)).all(axis=1)
    assert (strictly & edge).any()
    rmse = lambda c, at: float(np.sqrt(((c[at].astype(np.float64) - truth[at]) ** 2).mean()))
    figures = {}
    for what, at in (("floor", floor), ("inside a cell", inside), ("at a cell edge", edge)):
        arms = (rmse(without["noisy"][:, 0:3], at), rmse(without["records"][:, 0:3], at), rmse(with_centre["records"][:, 0:3], at), rmse(with_mean["records"][:, 0:3], at))
        figures[what] = arms
        print(f"checkered floor, {what}, {int(at.sum())} pixels, RMSE against 512 samples: raw {arms[0]:.6f}, filter without albedo {arms[1]:.6f}, "
              f"with the pixel-centre albedo {arms[2]:.6f}, with the mean albedo {arms[3]:.6f}")
    assert np.isfinite(np.array(list(figures.values()))).all()
    assert figures["at a cell edge"][3] < figures["at a cell edge"][2], figures["at a cell edge"]
