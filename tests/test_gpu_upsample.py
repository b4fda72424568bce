"""rr_upsample_records on the device against the numpy yardstick rustray_amd/upsample.py, every output word equal.

1: the hand-made frames of tests/upsample_cases.py at the shapes where the kernel can go wrong -- 37x19 <- 19x10 (a ratio that is no whole
number, two workgroups across), 65x17 <- 17x5 (a patch wider than the tile is not needed: ratio 3.8), 9x1 <- 3x1, 1x1 <- 1x1, 33x9 <- 33x9
(the 34-column patch), 64x48 <- 32x24 (several workgroups both ways) -- with and without halves and albedo, each optional output NULL,
sentinels behind every output, powers 0 and 7; 2: the host form against the device form; 3: a real scene end to end, holes filled; 4: the
ids against the frame's own; 5: behind its producer on a stream, the frames around the call unchanged; 6: the C++ layer."""
import ctypes as C

import numpy as np
import pytest

from rustray_amd import denoise, upsample
from rustray_amd.flat import make_config
from rustray_amd.upsample import UpsampleParams, upsample_records
from tests.denoise_cases import F, differing_words
from tests.helpers import camera_for, load_scene
from tests.test_gpu_pixel_parts import SENTINEL
from tests.upsample_cases import GPU_SHAPES, random_case

pytestmark = pytest.mark.gpu

_want = {}


def _yardstick(shape, use_halves, prm: UpsampleParams):
    """The yardstick's answer for random_case(*shape), computed once per case and left unchanged."""
    key = (shape, use_halves, prm.normal_power_log2, prm.sigma_depth, bool(prm.use_albedo))
    if key not in _want:
        W, H, w, h = shape
        low, halves, guide_low, guide = random_case(W, H, w, h)
        res = upsample_records(low, halves if use_halves else None, guide_low, guide, w, h, W, H, prm)
        res["rgba"] = denoise.frame_bytes_linear(res["records"][:, 0:3])    # the byte rule rr_denoise_records' rgba8_out is held to
        _want[key] = res
    return _want[key]


@pytest.fixture(scope="module")
def small_scene(hip):
    with hip.DeviceScene(load_scene("spheres_room"), 0) as ds:      # any small scene gives the handle
        yield ds


def _device_call(ds, shape, use_halves, prm, rgba8=True, weight=True, stream=None, produce=False):
    """One rr_upsample_records_device call on random_case(*shape) with sentinels in and behind every output, requested or not ->
    (records, halves, weight, rgba) as numpy words.  produce: the inputs are made by copy kernels on `stream` and the call follows them
    without a synchronisation."""
    import torch
    W, H, w, h = shape
    n = W * H
    inputs = random_case(W, H, w, h)
    ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.device(0)
    with ctx:
        src = [torch.from_numpy(a.copy().view(np.uint32).reshape(len(a), -1).view(np.int32)).cuda() for a in inputs]
        torch.cuda.synchronize()
        if produce:
            src = [t.clone() for t in src]          # (copy kernels on `stream`; the call is enqueued behind them)
        low_t, hv_t, gl_t, gf_t = src
        full = lambda words: torch.full((n + 2, words), SENTINEL, dtype=torch.int32, device="cuda")
        out, hout, wt, rgba = full(8), full(16), full(1), full(1)
        if not produce:
            torch.cuda.synchronize()
        ds.upsample_device(w, h, W, H, low_t.data_ptr(), hv_t.data_ptr() if use_halves else None, gl_t.data_ptr(), gf_t.data_ptr(), out.data_ptr(),
                           hout.data_ptr() if use_halves else None, rgba.data_ptr() if rgba8 else None, wt.data_ptr() if weight else None, prm,
                           stream.cuda_stream if stream is not None else None)
    torch.cuda.synchronize()
    o, ho, wo, r = (t.cpu().numpy().view(np.uint32) for t in (out, hout, wt, rgba))
    for name, a in (("out", o), ("halves_out", ho), ("weight_out", wo), ("rgba8_out", r)):
        assert (a[n:] == SENTINEL).all(), f"words behind {name} were written"
    for name, a, asked in (("halves_out", ho, use_halves), ("weight_out", wo, weight), ("rgba8_out", r, rgba8)):
        assert asked or (a == SENTINEL).all(), f"{name} was not requested and was written"
    for t, a in zip(src, inputs):                   # the inputs are what they were
        assert np.array_equal(t.cpu().numpy().view(np.uint32).reshape(-1), a.view(np.uint32).reshape(-1))
    return o[:n], ho[:n].reshape(n, 2, 8), wo[:n, 0], r[:n, 0].copy().view(np.uint8).reshape(n, 4)


def _check(got, want, what, use_halves=True, rgba8=True, weight=True):
    rec, hv, wt, rgba = got
    w = want["records"].view(np.uint32)
    assert np.array_equal(rec, w), f"{what}: {int((rec != w).sum())} of {w.size} record words differ (first pixel {int(np.argwhere((rec != w).any(1))[0][0])})"
    if use_halves:
        # a half colour that is not finite propagates, and a NaN the arithmetic makes of it (0 * inf, a sum of two NaNs) has no specified
        # sign or payload: such words must be NaNs on both sides; every other word is held to bits
        differ, nans = differing_words(hv, want["halves"])
        assert differ == 0, f"{what}: {differ} half words differ ({nans} are NaNs of other bits on both sides)"
    if weight:
        assert np.array_equal(wt, want["weight"].view(np.uint32)), f"{what}: {int((wt != want['weight'].view(np.uint32)).sum())} weights differ"
    if rgba8:
        assert np.array_equal(rgba, want["rgba"]), f"{what}: {int((rgba != want['rgba']).sum())} bytes differ"


# ---- 1: hand-made frames against the yardstick --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", GPU_SHAPES, ids=lambda s: "%dx%d_from_%dx%d" % s)
def test_every_word_equals_the_yardstick(small_scene, shape):
    prm = UpsampleParams()
    _check(_device_call(small_scene, shape, True, prm), _yardstick(shape, True, prm), str(shape))


@pytest.mark.parametrize("shape", (GPU_SHAPES[0], GPU_SHAPES[5]), ids=lambda s: "%dx%d_from_%dx%d" % s)
def test_variants_and_optional_outputs(small_scene, shape):
    for use_halves, use_albedo, power in ((False, True, 5), (True, False, 5), (False, False, 0), (True, True, 0), (True, True, 7)):
        prm = UpsampleParams(normal_power_log2=power, sigma_depth=0.05 if power else 0.3, use_albedo=use_albedo)
        _check(_device_call(small_scene, shape, use_halves, prm), _yardstick(shape, use_halves, prm), f"{shape} halves={use_halves} albedo={use_albedo} power {power}",
               use_halves=use_halves)
    prm = UpsampleParams()
    want = _yardstick(shape, True, prm)
    _check(_device_call(small_scene, shape, True, prm, rgba8=False), want, f"{shape} without rgba8_out", rgba8=False)
    _check(_device_call(small_scene, shape, True, prm, weight=False), want, f"{shape} without weight_out", weight=False)
    _check(_device_call(small_scene, shape, False, prm, rgba8=False, weight=False), _yardstick(shape, False, prm), f"{shape} out alone", use_halves=False, rgba8=False,
           weight=False)


# ---- 2: the two forms, streams ------------------------------------------------------------------------------------------------------
def test_host_form_equals_device_form(small_scene):
    shape = GPU_SHAPES[0]
    W, H, w, h = shape
    prm = UpsampleParams(sigma_depth=0.1)
    low, halves, guide_low, guide = random_case(W, H, w, h)
    host = small_scene.upsample(w, h, W, H, low, guide_low, guide, halves, prm, rgba8=True)
    dev = _device_call(small_scene, shape, True, prm)
    assert np.array_equal(host["records"].view(np.uint32), dev[0]) and np.array_equal(host["halves"].view(np.uint32), dev[1])
    assert np.array_equal(host["weight"].view(np.uint32), dev[2]) and np.array_equal(host["rgba"], dev[3])
    _check((host["records"].view(np.uint32), host["halves"].view(np.uint32), host["weight"].view(np.uint32), host["rgba"]), _yardstick(shape, True, prm), "host form")
    plain = small_scene.upsample(w, h, W, H, low, guide_low, guide, None, prm, weight=False)
    assert plain["halves"] is None and np.array_equal(plain["records"].view(np.uint32), dev[0])
    # gamma_correction reaches the bytes only
    g = small_scene.upsample(w, h, W, H, low, guide_low, guide, halves, UpsampleParams(sigma_depth=0.1, gamma_correction=True), rgba8=True)
    assert np.array_equal(g["records"].view(np.uint32), host["records"].view(np.uint32)) and not np.array_equal(g["rgba"], host["rgba"])


def test_behind_its_producer_and_the_frames_around_it_are_the_same(hip):
    """The inputs come from copy kernels on a non-null stream and the call follows them without a synchronisation; the handle renders the
    same frame before and after, and nothing of a frame's statistics is touched."""
    import torch
    fs = load_scene("spheres_room")
    cam = camera_for(fs, 50, 38).c_struct()
    cfg = make_config(samples=2, monte_carlo=True, seed=3, max_recursion=4)
    prm = UpsampleParams()
    st = torch.cuda.Stream()
    with hip.DeviceScene(fs, 0) as ds:
        first = ds.render(cam, cfg, aux=True)
        stats = ds.stats()
        for shape in (GPU_SHAPES[5], GPU_SHAPES[0]):
            _check(_device_call(ds, shape, True, prm, stream=st, produce=True), _yardstick(shape, True, prm), f"{shape} behind its producer")
        assert ds.stats() == stats
        second = ds.render(cam, cfg, aux=True)
        for k in ("rgba", "normal", "depth", "object_id"):
            assert np.array_equal(first[k], second[k], equal_nan=True), k


# ---- 3, 4: a real scene -----------------------------------------------------------------------------------------------------------------
W, H, LW, LH = 64, 48, 32, 24


@pytest.fixture(scope="module")
def spheres(hip):
    from rustray_amd.renderer import Raytracing
    fs = load_scene("spheres")
    rt = Raytracing(fs, camera_for(fs, W, H), 0)
    rt.config = make_config(samples=4, monte_carlo=True, seed=3, max_recursion=4)
    yield rt
    rt.device_scene.close()


@pytest.fixture(scope="module")
def room(hip):
    from rustray_amd.renderer import Raytracing
    fs = load_scene("spheres_room")
    rt = Raytracing(fs, camera_for(fs, W, H), 0)
    rt.config = make_config(samples=4, monte_carlo=True, seed=3, max_recursion=4)
    yield rt
    rt.device_scene.close()


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_render_upsampled_equals_the_calls_one_by_one(spheres):
    """spheres at 64x48 <- 32x24: Raytracing.render_upsampled is render_pixel_parts on the small camera, surface_pixels on both and the
    yardstick, bit for bit; the torch form, on one stream with no host trip, gives the same; with denoise_params the filter follows."""
    import torch
    from rustray_amd import renderer
    from rustray_amd.renderer import _low_camera, _pack_records
    rt = spheres
    ds, cam = rt.device_scene, rt.camera.c_struct()
    low_cam, w, h = _low_camera(cam, 2)
    assert (w, h) == (LW, LH)
    base = ds.render_pixel_parts(low_cam, rt.config, n_parts=2)
    low, halves_low = _pack_records(base), _pack_records(base["parts"])
    guide_low, guide = ds.surface_pixels(low_cam, albedo=False), ds.surface_pixels(cam, albedo=False)
    assert 0.05 < (guide["hit"] != 0).mean() < 0.95           # hits and misses both
    want = upsample_records(low, halves_low, guide_low, guide, w, h, W, H)
    got = rt.render_upsampled(scale=2, rgba8=True)
    assert np.array_equal(_words(got["records"]), _words(want["records"])), int((_words(got["records"]) != _words(want["records"])).sum())
    assert np.array_equal(_words(got["halves"]), _words(want["halves"])) and np.array_equal(_words(got["weight"]), _words(want["weight"]))
    assert np.array_equal(got["rgba"], denoise.frame_bytes_linear(want["records"][:, 0:3])) and got["count"] == 0 and (got["low_width"], got["low_height"]) == (w, h)
    t = renderer.render_upsampled_torch(ds, cam, rt.config, scale=2, rgba8=True)
    torch.cuda.synchronize()
    assert np.array_equal(_words(t["records"].cpu().numpy()), _words(want["records"])) and np.array_equal(_words(t["halves"].cpu().numpy()), _words(want["halves"]))
    assert np.array_equal(_words(t["weight"].cpu().numpy()), _words(want["weight"])) and np.array_equal(t["rgba"].cpu().numpy(), got["rgba"])
    assert np.array_equal(_words(t["low"].cpu().numpy()), _words(low)) and np.array_equal(_words(t["guide"].cpu().numpy()).reshape(-1), _words(guide).reshape(-1))
    # the guide fields of a missed pixel are the bits rr_render_pixels writes for a pixel all of whose rays missed
    full = _pack_records(ds.render_pixels(cam, rt.config))
    all_miss = np.isnan(full[:, 4]) & (guide["hit"] == 0)
    assert all_miss.sum() > 0.3 * W * H
    assert np.array_equal(_words(want["records"][all_miss, 3:]), _words(full[all_miss, 3:]))
    # with the filter behind it: rr_denoise_records at full size on the upsampled records and halves, the full guide's albedo
    dprm = denoise.DenoiseParams(iterations=3)
    albedo = np.ascontiguousarray(guide["base_color"][:, 0:3])
    filtered = denoise.atrous_denoise(want["records"], want["halves"], albedo, W, H, dprm)
    got_d = rt.render_upsampled(scale=2, denoise_params=dprm)
    assert np.array_equal(_words(got_d["records"]), _words(filtered["records"])) and np.array_equal(_words(got_d["upsampled"]), _words(want["records"]))
    t_d = renderer.render_upsampled_torch(ds, cam, rt.config, scale=2, denoise_params=dprm)
    torch.cuda.synchronize()
    assert np.array_equal(_words(t_d["records"].cpu().numpy()), _words(filtered["records"]))


@pytest.mark.parametrize("scale", (2, 4))
def test_fill_holes_changes_exactly_the_listed_pixels(room, scale):
    """fill_holes=True: the pixels with weight 0 on a surface are traced at full resolution and become rr_render_pixels' bits (halves:
    rr_render_pixel_parts'); every other pixel keeps its upsampled bits; the count is in the result.  spheres_room, where every pixel
    is a hit, at 64x48 <- 32x24 and <- 16x12: the spheres fixture has no hole at 32x24 (the CPU oracle's closest hits: 0 there, 2 here)."""
    import torch
    from rustray_amd import renderer
    from rustray_amd.renderer import _pack_records
    rt = room
    ds, cam = rt.device_scene, rt.camera.c_struct()
    plain = rt.render_upsampled(scale=scale)
    guide = ds.surface_pixels(cam, albedo=False)
    listed = (plain["weight"] == 0) & (guide["hit"] != 0)
    assert listed.sum() > 0, "the fixture has no hole: the test shows nothing"
    fine = ds.render_pixel_parts(cam, rt.config, n_parts=2)
    full = _pack_records(ds.render_pixels(cam, rt.config))
    assert np.array_equal(_words(full), _words(_pack_records(fine)))
    for got in (rt.render_upsampled(scale=scale, fill_holes=True), renderer.render_upsampled_torch(ds, cam, rt.config, scale=scale, fill_holes=True)):
        torch.cuda.synchronize()
        rec, hv = (np.asarray(got[k].cpu().numpy() if hasattr(got[k], "cpu") else got[k]) for k in ("records", "halves"))
        holes = np.asarray(got["holes"].cpu().numpy() if hasattr(got["holes"], "cpu") else got["holes"]).view(np.uint32)
        assert got["count"] == int(listed.sum()) == len(holes)
        assert np.array_equal(np.sort((holes & 0xffff) + (holes >> 16) * W), np.flatnonzero(listed))
        assert np.array_equal(_words(rec[listed]), _words(full[listed])) and np.array_equal(_words(hv[listed]), _words(_pack_records(fine["parts"])[listed]))
        assert np.array_equal(_words(rec[~listed]), _words(plain["records"][~listed])) and np.array_equal(_words(hv[~listed]), _words(plain["halves"][~listed]))


def test_object_ids_are_the_frames_own(room):
    """spheres_room at 64x48 <- 32x24: out.object_id equals the id of the full-resolution rr_render_pixels record on every pixel whose 3x3
    G-buffer neighbourhood is one hit item (a frame's id is its last sample's, which falls inside the pixel).  Those pixels are three
    quarters of this frame (the CPU oracle's closest hits of the pixel-centre rays: 0.7507); under half, the test would show little."""
    rt = room
    got = rt.render_upsampled(scale=2)
    full = rt.render_pixels()
    guide = rt.surface_pixels()
    ids = np.where(guide["hit"] != 0, guide["object_id"].astype(np.int64), -1).reshape(H, W)
    one = np.zeros((H, W), bool)
    one[1:-1, 1:-1] = ids[1:-1, 1:-1] >= 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            one[1:-1, 1:-1] &= ids[1 + dy:H - 1 + dy, 1 + dx:W - 1 + dx] == ids[1:-1, 1:-1]
    one = one.reshape(-1)
    assert one.mean() >= 0.5, f"only {one.mean():.3f} of the frame lies inside one item"
    assert np.array_equal(got["object_id"][one], full["object_id"][one])
    assert np.array_equal(got["object_id"], np.where(guide["hit"] != 0, guide["object_id"], 0))


# ---- 6: the C++ layer ---------------------------------------------------------------------------------------------------------------
def test_upsample_through_the_cpp_host_layer(hip):
    from tests.test_cpp_host import _cam_args
    from tests.test_gpu_pixel_parts_cpp import _shim
    shape = GPU_SHAPES[0]
    Wc, Hc, w, h = shape
    n = Wc * Hc
    low, halves, guide_low, guide = random_case(*shape)
    prm = UpsampleParams(normal_power_log2=2, sigma_depth=0.2)
    want = _yardstick(shape, True, prm)
    fs = load_scene("spheres_room")
    camera = camera_for(fs, Wc, Hc)
    cfg = make_config(samples=2, monte_carlo=True, seed=3, max_recursion=4)
    L = _shim()
    cam_types = list(L.rh_render_pixel_parts.argtypes[1:10])
    L.rh_upsample.argtypes = [C.c_void_p] + cam_types + [C.c_uint32, C.c_uint32] + [C.c_void_p] * 9
    cs = fs.c_struct()
    handle = L.rh_scene_create(C.byref(cs), 0)
    assert handle
    args = _cam_args(camera) + (C.byref(cfg), Wc, Hc)
    try:
        out, hout, wt, rgba = np.zeros((n, 8), F), np.zeros((n, 2, 8), F), np.zeros(n, F), np.zeros((n, 4), np.uint8)
        cprm = hip.upsample_params(prm)
        assert L.rh_upsample(handle, *args, w, h, low.ctypes.data, halves.ctypes.data, guide_low.ctypes.data, guide.ctypes.data, C.addressof(cprm), out.ctypes.data,
                             hout.ctypes.data, wt.ctypes.data, rgba.ctypes.data) == 0
        _check((_words(out), _words(hout), _words(wt), rgba), want, "through the C++ layer")
        cprm.normal_power_log2 = 8
        assert L.rh_upsample(handle, *args, w, h, low.ctypes.data, None, guide_low.ctypes.data, guide.ctypes.data, C.addressof(cprm), out.ctypes.data, None, None, None) == -1
        assert b"normal_power_log2" in hip.lib().rr_last_error()
    finally:
        L.rh_scene_destroy(handle)
