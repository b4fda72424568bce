"""rr_upsample_albedo_records on the device against the numpy yardstick rustray_amd/upsample.py, every output word equal.

1: the hand-made frames of tests/upsample_cases.py with the planes of tests/upsample_albedo_cases.py at the shapes where the kernel can go
wrong (several tiles each way, ragged last tiles, a ratio that is no whole number, ratio 1, one pixel), the low plane alone, the full one
alone and both, sentinels in and behind every output; 2: planes at an address that is 4-byte and not 16-byte aligned, between huge finite
floats; 3: both planes NULL against rr_upsample_records_device; 4: the host form; 5: behind its producer on a stream; 6: the pipelines
against the calls one by one and the yardsticks; 7: the C++ layer."""
import ctypes as C

import numpy as np
import pytest

from rustray_amd import denoise
from rustray_amd.flat import make_config
from rustray_amd.upsample import UpsampleParams, upsample_records
from tests.denoise_cases import F, differing_words
from tests.helpers import camera_for, load_scene
from tests.test_gpu_pixel_parts import SENTINEL
from tests.upsample_albedo_cases import PLANE_SETS, random_planes
from tests.upsample_cases import GPU_SHAPES, random_case

pytestmark = pytest.mark.gpu

HUGE = F(3.0e38)       # around a plane: finite, so a load that strays shows in a colour and not as one more NaN
ids = lambda s: "%dx%d_from_%dx%d" % s
_want = {}


def _planes(shape, with_low, with_full):
    al, af = random_planes(*shape)
    return (al if with_low else None), (af if with_full else None)


def _yardstick(shape, use_halves, prm: UpsampleParams, with_low, with_full):
    """The yardstick's answer for random_case(*shape) with random_planes(*shape), computed once per case and left unchanged."""
    key = (shape, use_halves, prm.normal_power_log2, prm.sigma_depth, bool(prm.use_albedo), with_low, with_full)
    if key not in _want:
        W, H, w, h = shape
        low, halves, guide_low, guide = random_case(W, H, w, h)
        al, af = _planes(shape, with_low, with_full)
        res = upsample_records(low, halves if use_halves else None, guide_low, guide, w, h, W, H, prm, albedo_low=al, albedo=af)
        res["rgba"] = denoise.frame_bytes_linear(res["records"][:, 0:3])
        _want[key] = res
    return _want[key]


@pytest.fixture(scope="module")
def small_scene(hip):
    with hip.DeviceScene(load_scene("spheres_room"), 0) as ds:      # any small scene gives the handle
        yield ds


def _device_call(ds, shape, use_halves, prm, with_low, with_full, lead=4, stream=None, produce=False, old_symbol=False, outputs=True):
    """One rr_upsample_albedo_records_device call on random_case(*shape) and its planes, with sentinels in and behind every output,
    requested or not -> (records, halves, weight, rgba) as numpy words.  A plane lies `lead` floats into a tensor of HUGE floats that goes
    on behind it (lead 4: 16-byte aligned; lead 1: 4-byte aligned and no more).  produce: the inputs and planes are made by copy kernels on
    `stream` and the call follows them without a synchronisation.  outputs=False: rgba8_out and weight_out are NULL.  old_symbol:
    rr_upsample_records_device, which takes no planes."""
    import torch
    W, H, w, h = shape
    n = W * H
    inputs = random_case(W, H, w, h)
    planes = _planes(shape, with_low, with_full)
    ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.device(0)
    with ctx:
        src = [torch.from_numpy(a.copy().view(np.uint32).reshape(len(a), -1).view(np.int32)).cuda() for a in inputs]
        held = []
        for a in planes:
            if a is None:
                held.append(None)
                continue
            host = np.full(lead + a.size + 5, HUGE, F)
            host[lead:lead + a.size] = a.reshape(-1)
            held.append(torch.from_numpy(host).cuda())
        torch.cuda.synchronize()
        if produce:
            src = [t.clone() for t in src]          # (copy kernels on `stream`; the call is enqueued behind them)
            held = [None if t is None else t.clone() for t in held]
        low_t, hv_t, gl_t, gf_t = src
        views = [None if t is None else t[lead:lead + a.size] for t, a in zip(held, planes)]
        for v in views:
            assert v is None or (v.data_ptr() % 4 == 0 and (v.data_ptr() % 16 == 0) == (lead % 4 == 0))
        full = lambda words: torch.full((n + 2, words), SENTINEL, dtype=torch.int32, device="cuda")
        out, hout, wt, rgba = full(8), full(16), full(1), full(1)
        if not produce:
            torch.cuda.synchronize()
        kw = {} if old_symbol else dict(albedo_low=views[0].data_ptr() if views[0] is not None else None, albedo=views[1].data_ptr() if views[1] is not None else None)
        fn = ds.upsample_device
        if not old_symbol and views[0] is None and views[1] is None:      # the new symbol with two NULLs (the binding would take the older one)
            from rustray_amd import capi
            p = capi.upsample_params(prm)
            fn = lambda lw, lh, fw, fh, lo, hv, gl, gf, o, ho, rg, wo, _prm, st, **_: capi._check(capi.lib().rr_upsample_albedo_records_device(
                ds._h, lw, lh, fw, fh, C.byref(p), *(capi._ptr(x) for x in (lo, hv, gl, gf, None, None, o, ho, rg, wo, st))))
        fn(w, h, W, H, low_t.data_ptr(), hv_t.data_ptr() if use_halves else None, gl_t.data_ptr(), gf_t.data_ptr(), out.data_ptr(),
           hout.data_ptr() if use_halves else None, rgba.data_ptr() if outputs else None, wt.data_ptr() if outputs else None, prm,
           stream.cuda_stream if stream is not None else None, **kw)
    torch.cuda.synchronize()
    o, ho, wo, r = (t.cpu().numpy().view(np.uint32) for t in (out, hout, wt, rgba))
    for name, a in (("out", o), ("halves_out", ho), ("weight_out", wo), ("rgba8_out", r)):
        assert (a[n:] == SENTINEL).all(), f"words behind {name} were written"
    for name, a, asked in (("halves_out", ho, use_halves), ("weight_out", wo, outputs), ("rgba8_out", r, outputs)):
        assert asked or (a == SENTINEL).all(), f"{name} was not requested and was written"
    for t, a in zip(src, inputs):                   # the inputs are what they were
        assert np.array_equal(t.cpu().numpy().view(np.uint32).reshape(-1), a.view(np.uint32).reshape(-1))
    for t, a in zip(held, planes):
        if t is not None:
            back = t.cpu().numpy()
            assert np.array_equal(back[lead:lead + a.size].view(np.uint32), a.reshape(-1).view(np.uint32))
            assert (back[:lead] == HUGE).all() and (back[lead + a.size:] == HUGE).all()
    return o[:n], ho[:n].reshape(n, 2, 8), wo[:n, 0], r[:n, 0].copy().view(np.uint8).reshape(n, 4)


def _check(got, want, what, use_halves=True, outputs=True):
    rec, hv, wt, rgba = got
    w = want["records"].view(np.uint32)
    assert np.array_equal(rec, w), f"{what}: {int((rec != w).sum())} of {w.size} record words differ (first pixel {int(np.argwhere((rec != w).any(1))[0][0])})"
    if use_halves:
        differ, nans = differing_words(hv, want["halves"])
        assert differ == 0, f"{what}: {differ} half words differ ({nans} are NaNs of other bits on both sides)"
    if not outputs:
        return
    assert np.array_equal(wt, want["weight"].view(np.uint32)), f"{what}: {int((wt != want['weight'].view(np.uint32)).sum())} weights differ"
    assert np.array_equal(rgba, want["rgba"]), f"{what}: {int((rgba != want['rgba']).sum())} bytes differ"


# ---- 1: hand-made frames against the yardstick --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", GPU_SHAPES, ids=ids)
def test_every_word_equals_the_yardstick(small_scene, shape):
    prm = UpsampleParams()
    for name, with_low, with_full in PLANE_SETS:
        _check(_device_call(small_scene, shape, True, prm, with_low, with_full), _yardstick(shape, True, prm, with_low, with_full), f"{shape} planes={name}")


@pytest.mark.parametrize("shape", (GPU_SHAPES[0], GPU_SHAPES[5]), ids=ids)
def test_variants(small_scene, shape):
    for use_halves, use_albedo, power in ((False, True, 5), (True, True, 0), (False, True, 7), (True, False, 5), (False, False, 0)):
        prm = UpsampleParams(normal_power_log2=power, sigma_depth=0.05 if power else 0.3, use_albedo=use_albedo)
        for name, with_low, with_full in PLANE_SETS:
            _check(_device_call(small_scene, shape, use_halves, prm, with_low, with_full), _yardstick(shape, use_halves, prm, with_low, with_full),
                   f"{shape} halves={use_halves} albedo={use_albedo} power {power} planes={name}", use_halves=use_halves)
    prm = UpsampleParams()
    _check(_device_call(small_scene, shape, False, prm, True, True, outputs=False), _yardstick(shape, False, prm, True, True), f"{shape} out alone", use_halves=False,
           outputs=False)


# ---- 2: planes that are 4-byte aligned and no more ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", (GPU_SHAPES[0], GPU_SHAPES[1]), ids=ids)
def test_planes_at_an_address_that_is_not_16_byte_aligned(small_scene, shape):
    """A view one float into a larger tensor, a huge finite float before and behind it: a load wider than a plane's alignment allows, or
    one that strays past either end, would put that float into a colour."""
    prm = UpsampleParams()
    for use_halves in (True, False):
        for name, with_low, with_full in PLANE_SETS:
            _check(_device_call(small_scene, shape, use_halves, prm, with_low, with_full, lead=1), _yardstick(shape, use_halves, prm, with_low, with_full),
                   f"{shape} halves={use_halves} planes={name}, one float in", use_halves=use_halves)


# ---- 3: both planes NULL --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", (GPU_SHAPES[0], GPU_SHAPES[5]), ids=ids)
def test_both_planes_null_is_the_older_call(small_scene, shape):
    prm = UpsampleParams()
    for use_halves in (True, False):
        new = _device_call(small_scene, shape, use_halves, prm, False, False)
        old = _device_call(small_scene, shape, use_halves, prm, False, False, old_symbol=True)
        for a, b, what in zip(new, old, ("records", "halves", "weight", "rgba")):
            assert np.array_equal(a, b), f"{shape} halves={use_halves}: {what}"
        _check(new, _yardstick(shape, use_halves, prm, False, False), f"{shape} two NULLs", use_halves=use_halves)


# ---- 4, 5: the two forms, streams -------------------------------------------------------------------------------------------------------
def test_host_form_equals_device_form(small_scene):
    shape = GPU_SHAPES[0]
    W, H, w, h = shape
    prm = UpsampleParams(sigma_depth=0.1)
    low, halves, guide_low, guide = random_case(W, H, w, h)
    for name, with_low, with_full in PLANE_SETS:
        al, af = _planes(shape, with_low, with_full)
        host = small_scene.upsample(w, h, W, H, low, guide_low, guide, halves, prm, rgba8=True, albedo_low=al, albedo=af)
        dev = _device_call(small_scene, shape, True, prm, with_low, with_full)
        got = (host["records"].view(np.uint32), host["halves"].view(np.uint32), host["weight"].view(np.uint32), host["rgba"])
        assert np.array_equal(got[0], dev[0]) and differing_words(got[1], dev[1])[0] == 0 and np.array_equal(got[2], dev[2]) and np.array_equal(got[3], dev[3]), name
        _check(got, _yardstick(shape, True, prm, with_low, with_full), f"host form, planes={name}")


def test_behind_its_producer_and_the_frames_around_it_are_the_same(hip):
    """The inputs and the planes come from copy kernels on a non-null stream and the call follows them without a synchronisation; the
    handle renders the same frame before and after, and nothing of a frame's statistics is touched."""
    import torch
    fs = load_scene("spheres_room")
    cam = camera_for(fs, 50, 38).c_struct()
    cfg = make_config(samples=2, monte_carlo=True, seed=3, max_recursion=4)
    prm = UpsampleParams()
    st = torch.cuda.Stream()
    shape = GPU_SHAPES[5]
    with hip.DeviceScene(fs, 0) as ds:
        first = ds.render(cam, cfg, aux=True)
        stats = ds.stats()
        for lead in (4, 1):
            _check(_device_call(ds, shape, True, prm, True, True, lead=lead, stream=st, produce=True), _yardstick(shape, True, prm, True, True),
                   f"{shape} behind its producer, lead {lead}")
        assert ds.stats() == stats
        second = ds.render(cam, cfg, aux=True)
        for k in ("rgba", "normal", "depth", "object_id"):
            assert np.array_equal(first[k], second[k], equal_nan=True), k


# ---- 6: the pipelines ---------------------------------------------------------------------------------------------------------------------
W, H, LW, LH = 64, 48, 32, 24


@pytest.fixture(scope="module")
def room(hip):
    from rustray_amd.renderer import Raytracing
    fs = load_scene("spheres_room")
    rt = Raytracing(fs, camera_for(fs, W, H), 0)
    rt.config = make_config(samples=4, monte_carlo=True, seed=3, max_recursion=4)
    yield rt
    rt.device_scene.close()


def _words(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else a
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def pieces(room):
    """The calls of the pipelines one by one, made once: the low frame, both guides, the mean planes."""
    from rustray_amd.renderer import _config_at, _low_camera, _pack_records
    rt = room
    ds, cam = rt.device_scene, rt.camera.c_struct()
    low_cam, w, h = _low_camera(cam, 2)
    assert (w, h) == (LW, LH)
    base = ds.render_pixel_parts(low_cam, rt.config, n_parts=2)
    p = dict(low=_pack_records(base), halves_low=_pack_records(base["parts"]), guide_low=ds.surface_pixels(low_cam, albedo=False),
             guide=ds.surface_pixels(cam, albedo=False), mean_low=ds.albedo_pixels(low_cam, rt.config), mean_full=ds.albedo_pixels(cam, _config_at(rt.config, 2)))
    p["centre_low"] = np.ascontiguousarray(p["guide_low"]["base_color"][:, 0:3])
    p["centre_full"] = np.ascontiguousarray(p["guide"]["base_color"][:, 0:3])
    return p


LOW_FILTER, FULL_FILTER = denoise.DenoiseParams(iterations=2), denoise.DenoiseParams(iterations=3)
PIPELINES = (("mean", dict(albedo="mean")),
             ("mean_full", dict(albedo="mean", full_albedo_samples=2)),
             ("mean_full_lowfilter", dict(albedo="mean", full_albedo_samples=2, low_denoise_params=LOW_FILTER)),
             ("mean_full_lowfilter_filter", dict(albedo="mean", full_albedo_samples=2, low_denoise_params=LOW_FILTER, denoise_params=FULL_FILTER)),
             ("centre_lowfilter_filter", dict(low_denoise_params=LOW_FILTER, denoise_params=FULL_FILTER)))


def _recipe(p, albedo=True, full_albedo_samples=None, low_denoise_params=None, denoise_params=None):
    """What the pipeline must give, from the calls one by one and the yardsticks -> (upsampled dict, filtered records or None, planes)."""
    al = p["mean_low"] if albedo == "mean" else None
    af = p["mean_full"] if full_albedo_samples is not None else None
    low, halves_low = p["low"], p["halves_low"]
    if low_denoise_params is not None:
        low = denoise.atrous_denoise(low, halves_low, al if al is not None else p["centre_low"], LW, LH, low_denoise_params)["records"]
        halves_low = None
    up = upsample_records(low, halves_low, p["guide_low"], p["guide"], LW, LH, W, H, albedo_low=al, albedo=af)
    filtered = None
    if denoise_params is not None:
        filtered = denoise.atrous_denoise(up["records"], up["halves"], af if af is not None else p["centre_full"], W, H, denoise_params)["records"]
    return up, filtered, (al, af)


def test_the_mean_plane_is_not_the_centre_albedo(pieces):
    hit = pieces["guide_low"]["hit"] != 0
    differs = (pieces["mean_low"] != pieces["centre_low"]).any(1) & hit
    assert differs.any(), "the mean low plane is the low guide's centre albedo at every hit pixel: the pipeline tests would show nothing"
    assert ((pieces["mean_full"] != pieces["centre_full"]).any(1) & (pieces["guide"]["hit"] != 0)).any()


def test_the_default_call_is_what_it_was(room, pieces):
    import torch
    from rustray_amd import renderer
    want, _, _ = _recipe(pieces)
    for got in (room.render_upsampled(scale=2), renderer.render_upsampled_torch(room.device_scene, room.camera.c_struct(), room.config, scale=2)):
        torch.cuda.synchronize()
        assert np.array_equal(_words(got["records"]), _words(want["records"])) and np.array_equal(_words(got["halves"]), _words(want["halves"]))
        assert np.array_equal(_words(got["weight"]), _words(want["weight"])) and got["albedo_low"] is None and got["albedo"] is None


@pytest.mark.parametrize("name,kw", PIPELINES, ids=[p[0] for p in PIPELINES])
def test_pipelines_equal_the_calls_one_by_one(room, pieces, name, kw):
    import torch
    from rustray_amd import renderer
    up, filtered, planes = _recipe(pieces, **kw)
    for form, got in (("host", room.render_upsampled(scale=2, **kw)),
                      ("torch", renderer.render_upsampled_torch(room.device_scene, room.camera.c_struct(), room.config, scale=2, **kw))):
        torch.cuda.synchronize()
        what = f"{name}, {form} form"
        for key, plane in zip(("albedo_low", "albedo"), planes):
            assert (got[key] is None) == (plane is None), what
            assert plane is None or np.array_equal(_words(got[key]), _words(plane)), f"{what}: {key}"
        raised = got["upsampled"] if "denoise_params" in kw else got["records"]
        assert np.array_equal(_words(raised), _words(up["records"])), f"{what}: {int((_words(raised) != _words(up['records'])).sum())} record words differ"
        assert np.array_equal(_words(got["weight"]), _words(up["weight"])), what
        if up["halves"] is None:
            assert got["halves"] is None, what
        else:
            assert differing_words(_words(got["halves"]).view(F), up["halves"])[0] == 0, what
        if filtered is not None:
            assert np.array_equal(_words(got["records"]), _words(filtered)), f"{what}: the filtered records"


def test_fill_holes_behind_a_filtered_low_frame_writes_records_only(room, pieces):
    import torch
    from rustray_amd import renderer
    from rustray_amd.renderer import _pack_records
    kw = dict(albedo="mean", low_denoise_params=LOW_FILTER)
    up, _, _ = _recipe(pieces, **kw)
    listed = (up["weight"] == 0) & (pieces["guide"]["hit"] != 0)
    assert listed.sum() > 0, "the fixture has no hole: the test shows nothing"
    full = _pack_records(room.device_scene.render_pixels(room.camera.c_struct(), room.config))
    for got in (room.render_upsampled(scale=2, fill_holes=True, **kw),
                renderer.render_upsampled_torch(room.device_scene, room.camera.c_struct(), room.config, scale=2, fill_holes=True, **kw)):
        torch.cuda.synchronize()
        assert got["halves"] is None and got["count"] == int(listed.sum())
        rec = _words(got["records"])
        assert np.array_equal(rec[listed], _words(full)[listed]) and np.array_equal(rec[~listed], _words(up["records"])[~listed])


# ---- 7: the C++ layer ---------------------------------------------------------------------------------------------------------------------
def test_upsample_albedo_through_the_cpp_host_layer(hip, room):
    from tests.test_cpp_host import _cam_args
    from tests.test_gpu_pixel_parts_cpp import _shim
    shape = GPU_SHAPES[0]
    Wc, Hc, w, h = shape
    n = Wc * Hc
    low, halves, guide_low, guide = random_case(*shape)
    al, af = random_planes(*shape)
    prm = UpsampleParams(normal_power_log2=2, sigma_depth=0.2)
    fs = load_scene("spheres_room")
    camera = camera_for(fs, Wc, Hc)
    cfg = make_config(samples=2, monte_carlo=True, seed=3, max_recursion=4)
    L = _shim()
    cam_types = list(L.rh_render_pixel_parts.argtypes[1:10])
    L.rh_upsample_albedo.argtypes = [C.c_void_p] + cam_types + [C.c_uint32, C.c_uint32] + [C.c_void_p] * 11
    L.rh_render_upsampled_albedo.argtypes = [C.c_void_p] + cam_types + [C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p] + [C.c_void_p] * 3
    cs = fs.c_struct()
    handle = L.rh_scene_create(C.byref(cs), 0)
    assert handle
    args = _cam_args(camera) + (C.byref(cfg), Wc, Hc)
    try:
        cprm = hip.upsample_params(prm)
        for name, with_low, with_full in PLANE_SETS:
            out, hout, wt, rgba = np.zeros((n, 8), F), np.zeros((n, 2, 8), F), np.zeros(n, F), np.zeros((n, 4), np.uint8)
            assert L.rh_upsample_albedo(handle, *args, w, h, low.ctypes.data, halves.ctypes.data, guide_low.ctypes.data, guide.ctypes.data,
                                        al.ctypes.data if with_low else None, af.ctypes.data if with_full else None, C.addressof(cprm), out.ctypes.data, hout.ctypes.data,
                                        wt.ctypes.data, rgba.ctypes.data) == 0
            _check((_words(out), _words(hout), _words(wt), rgba), _yardstick(shape, True, prm, with_low, with_full), f"through the C++ layer, planes={name}")
        # the pipeline of the C++ layer against Python's, on the room fixture's camera and config
        rt = room
        args = _cam_args(rt.camera) + (C.byref(rt.config), W, H)
        lprm, dprm = hip.denoise_params(LOW_FILTER), hip.denoise_params(FULL_FILTER)
        for mean, k, low_filter, full_filter in ((1, 0, False, False), (1, 2, True, True), (0, 0, True, False)):
            kw = dict(albedo="mean" if mean else True, full_albedo_samples=k or None, low_denoise_params=LOW_FILTER if low_filter else None,
                      denoise_params=FULL_FILTER if full_filter else None)
            want = rt.render_upsampled(scale=2, **kw)
            out, wt = np.zeros((W * H, 8), F), np.zeros(W * H, F)
            assert L.rh_render_upsampled_albedo(handle, *args, 2, None, C.addressof(dprm) if full_filter else None, mean, k, C.addressof(lprm) if low_filter else None,
                                                out.ctypes.data, wt.ctypes.data, None) == 0
            assert np.array_equal(_words(out), _words(want["records"])) and np.array_equal(_words(wt), _words(want["weight"])), kw
    finally:
        L.rh_scene_destroy(handle)
