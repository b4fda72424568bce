"""rr_denoise_split_records on the GPU and albedo="diffuse" in the single-frame pipelines.

BITS: denoise_split equals denoise.atrous_denoise_split bit for bit on rich_scene(9119) at 8 samples, with and without albedo and halves;
its two identities (diffuse = 0: the plain filter; diffuse = the colour: the filter with the albedo) hold against rr_denoise_records on
the device, except for the sign of a zero; Python, torch and C++ albedo="diffuse" equal the chain render_pixel_split -> albedo_pixels ->
atrous_denoise_split; True, False and "mean" keep their bits; the temporal pipelines raise ValueError for "diffuse".

QUALITY (test_quality_on_a_checkered_floor): the floor and protocol of tests/test_gpu_denoise_mean_albedo.py -- 8 samples in two halves,
truth at 512, default parameters, RMSE of linear colour over the floor, inside a cell and at a cell edge -- with five arms: raw, plain
filter, pixel-centre albedo, mean albedo, split.  Every figure is printed; DESIGN.md section 8 item 22 holds those of one MI355X:
the floor (853 pixels) 0.042100 / 0.085182 / 0.218705 / 0.106973 / 0.048474; inside a cell (64) 0.000203 / 0.094109 / 0.068753 /
0.071278 / 0.005173; at a cell edge (789) 0.043774 / 0.084417 / 0.226557 / 0.109359 / 0.050380."""
import ctypes as C

import numpy as np
import pytest

from rustray_amd import renderer
from rustray_amd.denoise import DenoiseParams, atrous_denoise, atrous_denoise_split, frame_bytes_linear
from rustray_amd.renderer import Raytracing, TemporalState, _pack_records
from tests.helpers import camera_for
from tests.test_cpp_host import _cam_args
from tests.test_denoise_split_host import same_but_zero_sign
from tests.test_gpu_denoise_albedo import F, H, N, W, _cfg, _checkered_floor, _rich, _u32
from tests.test_gpu_pixel_parts_cpp import _shim

pytestmark = pytest.mark.gpu

_frame = {}


def _rich_frame(hip):
    """The frame every bit test reads, made once and left unchanged: records, halves, diffuse, diffuse halves, the mean albedo."""
    if not _frame:
        fs = _rich()
        camera = camera_for(fs, W, H)
        rt = Raytracing(fs, camera, 0)
        try:
            rt.config = _cfg()
            base = rt.render_pixel_split()
            mean = rt.mean_albedo()
            centre = rt.albedo()
        finally:
            rt.device_scene.close()
        _frame.update(fs=fs, camera=camera, records=_pack_records(base), halves=_pack_records(base["parts"]), diffuse=base["diffuse"],
                      diffuse_halves=base["diffuse_halves"], mean=mean, centre=centre)
        for a in _frame.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return _frame


@pytest.mark.parametrize("with_albedo", (True, False))
@pytest.mark.parametrize("with_halves", (True, False))
def test_bit_for_bit_the_yardstick(hip, with_halves, with_albedo):
    f = _rich_frame(hip)
    hv, dh = (f["halves"], f["diffuse_halves"]) if with_halves else (None, None)
    al = f["mean"] if with_albedo else None
    assert f["diffuse"].any() and not np.array_equal(f["diffuse"], f["records"][:, 0:3])
    want = atrous_denoise_split(f["records"], hv, f["diffuse"], dh, al, W, H)["records"]
    with hip.DeviceScene(f["fs"], 0) as ds:
        got = ds.denoise_split(W, H, f["records"], f["diffuse"], hv, dh, al, rgba8=True)
        in_place = ds.denoise_split(W, H, f["records"], f["diffuse"], hv, dh, al, in_place=True)
        short = ds.denoise_split(W, H, f["records"], f["diffuse"], hv, dh, al, params=DenoiseParams(iterations=2, gamma_correction=True), rgba8=True)
    differ = int((_u32(got["records"]) != _u32(want)).sum())
    assert differ == 0, f"{differ} of {want.size} words differ"
    assert np.array_equal(_u32(in_place["records"]), _u32(want))
    assert np.array_equal(_u32(short["records"]), _u32(atrous_denoise_split(f["records"], hv, f["diffuse"], dh, al, W, H, DenoiseParams(iterations=2))["records"]))
    assert np.array_equal(got["rgba"], frame_bytes_linear(want[:, 0:3])) and not np.array_equal(short["rgba"], got["rgba"])      # the bytes of `out`
    if with_albedo:      # the albedo does something, and not what it does to the whole colour
        assert not np.array_equal(_u32(want), _u32(atrous_denoise_split(f["records"], hv, f["diffuse"], dh, None, W, H)["records"]))
        assert not np.array_equal(_u32(want), _u32(atrous_denoise(f["records"], hv, al, W, H)["records"]))


def test_the_two_identities_against_rr_denoise_records(hip):
    f = _rich_frame(hip)
    rec, hv, al = f["records"], f["halves"], f["mean"]
    with hip.DeviceScene(f["fs"], 0) as ds:
        plain = ds.denoise_records(W, H, rec, hv, None)["records"]
        guided = ds.denoise_records(W, H, rec, hv, al)["records"]
        none = ds.denoise_split(W, H, rec, np.zeros((N, 3), F), hv, np.zeros((N, 2, 3), F), al)["records"]
        all_of_it = ds.denoise_split(W, H, rec, rec[:, 0:3], hv, hv[:, :, 0:3], al)["records"]
        # refusals of the call's own
        with pytest.raises(hip.RustrayHipError) as e:
            ds.denoise_split(W, H, rec, None, hv, f["diffuse_halves"], al)
        assert e.value.code == -1 and "diffuse is NULL" in str(e.value)
        with pytest.raises(hip.RustrayHipError) as e:
            ds.denoise_split(W, H, rec, f["diffuse"], hv, None, al)
        assert e.value.code == -1 and "given together or not at all" in str(e.value)
        with pytest.raises(hip.RustrayHipError) as e:
            ds.denoise_split(W, H, rec, f["diffuse"], None, f["diffuse_halves"], al)
        assert e.value.code == -1 and "given together or not at all" in str(e.value)
    assert same_but_zero_sign(none, plain)
    assert same_but_zero_sign(all_of_it, guided)
    assert not np.array_equal(_u32(plain), _u32(guided))


def test_render_denoised_diffuse_in_python_torch_and_cpp(hip):
    import torch
    f = _rich_frame(hip)
    fs, camera = f["fs"], f["camera"]
    records, halves, mean, centre = f["records"], f["halves"], f["mean"], f["centre"]
    want = atrous_denoise_split(records, halves, f["diffuse"], f["diffuse_halves"], mean, W, H)["records"]
    want_mean = atrous_denoise(records, halves, mean, W, H)["records"]
    want_centre = atrous_denoise(records, halves, centre, W, H)["records"]
    plain = atrous_denoise(records, halves, None, W, H)["records"]
    rt = Raytracing(fs, camera, 0)
    try:
        rt.config = _cfg()
        got = rt.render_denoised(albedo="diffuse", rgba8=True)
        assert np.array_equal(_u32(got["noisy"]), _u32(records)) and np.array_equal(_u32(got["albedo"]), _u32(mean))
        assert np.array_equal(_u32(got["diffuse"]), _u32(f["diffuse"])) and np.array_equal(_u32(got["diffuse_halves"]), _u32(f["diffuse_halves"]))
        differ = int((_u32(got["records"]) != _u32(want)).sum())
        assert differ == 0, differ
        assert got["rgba"].shape == (N, 4) and np.array_equal(_u32(got["color"]), _u32(want[:, 0:3]))
        # True, False and "mean" return what they returned before "diffuse" existed
        on, off, mid, default = rt.render_denoised(albedo=True), rt.render_denoised(albedo=False), rt.render_denoised(albedo="mean"), rt.render_denoised()
        assert np.array_equal(_u32(on["records"]), _u32(want_centre)) and np.array_equal(_u32(mid["records"]), _u32(want_mean))
        assert "albedo" not in off and np.array_equal(_u32(off["records"]), _u32(plain)) and np.array_equal(_u32(default["records"]), _u32(plain))
        assert "variance" in mid and "diffuse" not in mid
        # the temporal pipelines refuse it, before anything is rendered
        state = TemporalState()
        with pytest.raises(ValueError):
            rt.render_temporal(state, samples=4, albedo="diffuse")
        with pytest.raises(ValueError):
            renderer.render_temporal_torch(rt.device_scene, camera.c_struct(), rt.config, state, albedo="diffuse")
        assert state.frames == 0
        with pytest.raises(ValueError):
            rt.render_denoised(albedo="direct")
        # torch: three calls on one stream, no host trip
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            t = renderer.render_denoised_torch(rt.device_scene, camera.c_struct(), rt.config, albedo="diffuse", rgba8=True)
            t_mean = renderer.render_denoised_torch(rt.device_scene, camera.c_struct(), rt.config, albedo="mean")
            t_on = renderer.render_denoised_torch(rt.device_scene, camera.c_struct(), rt.config, albedo=True)
            t_off = renderer.render_denoised_torch(rt.device_scene, camera.c_struct(), rt.config, albedo=False)
        st.synchronize()
        assert t["records"].is_cuda and np.array_equal(_u32(t["records"]), _u32(want)) and np.array_equal(_u32(t["albedo"]), _u32(mean))
        assert np.array_equal(_u32(t["noisy"]), _u32(records)) and np.array_equal(_u32(t["halves"]), _u32(halves))
        assert np.array_equal(_u32(t["diffuse"]), _u32(f["diffuse"])) and np.array_equal(_u32(t["diffuse_halves"]), _u32(f["diffuse_halves"]))
        assert np.array_equal(t["rgba"].cpu().numpy(), got["rgba"])
        assert np.array_equal(_u32(t_mean["records"]), _u32(want_mean)) and np.array_equal(_u32(t_on["records"]), _u32(want_centre))
        assert "albedo" not in t_off and np.array_equal(_u32(t_off["records"]), _u32(plain))
    finally:
        rt.device_scene.close()
    # C++: Raytracing::render_denoised(AlbedoGuide::DIFFUSE, ...) through host_shim.cpp; MEAN, CENTRE and NONE keep their bits
    L = _shim()
    cam_types = list(L.rh_render_pixel_parts.argtypes[1:10])
    L.rh_render_denoised_diffuse.argtypes = [C.c_void_p] + cam_types + [C.c_void_p, C.c_void_p, C.c_void_p]
    L.rh_render_denoised_mean_albedo.argtypes = [C.c_void_p] + cam_types + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rh_render_denoised_albedo.argtypes = [C.c_void_p] + cam_types + [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    cs = fs.c_struct()
    h = L.rh_scene_create(C.byref(cs), 0)
    assert h
    cfg = _cfg()
    args = _cam_args(camera) + (C.byref(cfg), W, H)
    try:
        out, noisy = np.zeros((N, 8), F), np.zeros((N, 8), F)
        assert L.rh_render_denoised_diffuse(h, *args, None, out.ctypes.data, noisy.ctypes.data) == 0
        assert np.array_equal(_u32(noisy), _u32(records)) and np.array_equal(_u32(out), _u32(want))
        assert L.rh_render_denoised_mean_albedo(h, *args, None, out.ctypes.data, None, None) == 0
        assert np.array_equal(_u32(out), _u32(want_mean))
        assert L.rh_render_denoised_albedo(h, *args, None, 1, out.ctypes.data, None, None) == 0
        assert np.array_equal(_u32(out), _u32(want_centre))
        assert L.rh_render_denoised_albedo(h, *args, None, 0, out.ctypes.data, None, None) == 0
        assert np.array_equal(_u32(out), _u32(plain))
    finally:
        L.rh_scene_destroy(h)


def test_quality_on_a_checkered_floor(hip):
    """Five arms against the 512-sample truth over the floor's pixels (default parameters, 8 samples in two halves, monte_carlo on), split
    into the pixels whose 3x3 neighbourhood shows one checker colour under the pixels' centres and the ones at a colour edge; every figure
    is printed.  Asserted because it follows from the construction: all arms filtered the same noisy frame, the diffuse part of a floor
    pixel is a proper part of its colour (the floor has an ambient term), every figure is finite.  THE ASSERTION THE FEATURE AIMS FOR:
    over the floor the split arm's RMSE is below the mean-albedo arm's, both measured in this run.  Whether the split arm also beats the
    filter without an albedo is printed and not asserted: it decides a later change of the default."""
    fs = _checkered_floor()
    camera = camera_for(fs, W, H)
    rt = Raytracing(fs, camera, 0)
    try:
        rt.config = _cfg(samples=512)
        truth = rt.render_pixels()["color"].astype(np.float64)
        rt.config = _cfg(samples=8)
        split = rt.render_denoised(albedo="diffuse")
        with_mean = rt.render_denoised(albedo="mean")
        with_centre = rt.render_denoised(albedo=True)
        without = rt.render_denoised()
        surf = rt.surface_pixels()
    finally:
        rt.device_scene.close()
    floor = (surf["hit"] == 1) & (surf["object_id"] == 3)
    centre = with_centre["albedo"]
    assert floor.sum() > N // 4 and len(np.unique(centre[floor], axis=0)) == 2                      # both colours of the checker are in view
    for arm in (split, with_mean, with_centre):
        assert np.array_equal(_u32(arm["noisy"]), _u32(without["noisy"]))
    assert np.array_equal(_u32(split["albedo"]), _u32(with_mean["albedo"]))
    dif, col = split["diffuse"].astype(np.float64), without["noisy"][:, 0:3].astype(np.float64)
    assert (dif[floor] <= col[floor] + 2.0 ** -22).all() and (col[floor] - dif[floor] > 1e-3).any() and dif[floor].any()
    a = np.pad(centre[:, 0].reshape(H, W), 1, mode="edge")
    near = np.stack([a[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)])
    inside = ((near.max(0) == near.min(0)).reshape(N)) & floor
    edge = floor & ~inside
    rmse = lambda c, at: float(np.sqrt(((c[at].astype(np.float64) - truth[at]) ** 2).mean()))
    figures = {}
    for what, at in (("floor", floor), ("inside a cell", inside), ("at a cell edge", edge)):
        arms = (rmse(without["noisy"][:, 0:3], at), rmse(without["records"][:, 0:3], at), rmse(with_centre["records"][:, 0:3], at), rmse(with_mean["records"][:, 0:3], at),
                rmse(split["records"][:, 0:3], at))
        figures[what] = arms
        print(f"checkered floor, {what}, {int(at.sum())} pixels, RMSE against 512 samples: raw {arms[0]:.6f}, filter without albedo {arms[1]:.6f}, "
              f"with the pixel-centre albedo {arms[2]:.6f}, with the mean albedo {arms[3]:.6f}, split {arms[4]:.6f}")
    print(f"checkered floor: split {'beats' if figures['floor'][4] < figures['floor'][1] else 'does not beat'} the filter without an albedo over the floor")
    assert np.isfinite(np.array(list(figures.values()))).all()
    assert figures["floor"][4] < figures["floor"][3], figures["floor"]
