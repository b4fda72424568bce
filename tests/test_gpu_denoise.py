"""rr_denoise_records on the device against the numpy yardstick rustray_amd/denoise.py, every output word equal.

1: hand-made records (tests/denoise_cases.py; finite colours in [0, 2^10], so no sum overflows and NaNs only pass through) at the sizes
where the kernels take another path: 1x1 and 3x2, 5x5 at 6 iterations (every tap beyond the first ring outside), 37x19, 70x41 at 6
iterations (step 32), 130x70 (several workgroups both ways, tile seams at every step); with and without halves and albedo, in place, each
optional output NULL, sentinels behind every output, normal_power_log2 0 and 7; every form of the pass kernel; 2: the device form against
the host form, after its producer on a non-null stream, pageable memory refused by name; 3: the handle afterwards; 4: end to end on
spheres_room."""
import ctypes as C

import numpy as np
import pytest

from rustray_amd import denoise
from rustray_amd.denoise import DenoiseParams, atrous_denoise
from tests.denoise_cases import F, differing_words, random_frame
from tests.helpers import camera_for
from tests.test_gpu_pixel_parts import SENTINEL, _cfg
from tests.test_gpu_shade_rays import _scene

pytestmark = pytest.mark.gpu

_want = {}


def _yardstick(W, H, use_halves, use_albedo, prm: DenoiseParams):
    """The yardstick's answer for random_frame(W, H), computed once per case and left unchanged."""
    key = (W, H, use_halves, use_albedo, prm.iterations, prm.normal_power_log2, prm.sigma_depth, prm.sigma_luminance)
    if key not in _want:
        records, halves, albedo = random_frame(W, H)
        res = atrous_denoise(records, halves if use_halves else None, albedo if use_albedo else None, W, H, prm)
        res["rgba"] = denoise.frame_bytes_linear(res["records"][:, 0:3])
        _want[key] = res
    return _want[key]


@pytest.fixture(scope="module")
def small_scene(hip):
    with hip.DeviceScene(_scene("spheres_room"), 0) as ds:      # any small scene gives the handle
        yield ds


def _device_call(ds, W, H, use_halves, use_albedo, prm, in_place=False, rgba8=True, variance=True, stream=None, produce=False, frame=None):
    """One rr_denoise_records_device call on random_frame(W, H), or on `frame` = (records, halves, albedo) of that size, with sentinels
    behind every output -> (records, variance, rgba) as numpy words.  produce: the inputs are made by copy kernels on `stream` and the
    call follows them without a synchronisation."""
    import torch
    n = W * H
    records, halves, albedo = frame if frame is not None else random_frame(W, H)
    ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.device(0)
    with ctx:
        src = [torch.from_numpy(a.copy()).cuda() for a in (records, halves, albedo)]
        if produce:
            torch.cuda.synchronize()
            src = [t.clone() for t in src]          # (copy kernels on `stream`; the call is enqueued behind them)
        else:
            torch.cuda.synchronize()
        rec_t, hv_t, al_t = src
        if in_place:
            out = torch.full((n + 2, 8), SENTINEL, dtype=torch.int32, device="cuda")
            out[:n] = rec_t.view(torch.int32)
            rec_ptr = out.data_ptr()
            if not produce:
                torch.cuda.synchronize()
        else:
            out = torch.full((n + 2, 8), SENTINEL, dtype=torch.int32, device="cuda")
            rec_ptr = rec_t.data_ptr()
        rgba = torch.full((n + 2,), SENTINEL, dtype=torch.int32, device="cuda")
        var = torch.full((n + 2,), SENTINEL, dtype=torch.int32, device="cuda")
        if not produce:
            torch.cuda.synchronize()
        ds.denoise_records_device(W, H, rec_ptr, hv_t.data_ptr() if use_halves else None, al_t.data_ptr() if use_albedo else None, out.data_ptr(),
                                  rgba.data_ptr() if rgba8 else None, var.data_ptr() if variance else None, prm,
                                  stream.cuda_stream if stream is not None else None)
    torch.cuda.synchronize()
    o, r, v = out.cpu().numpy().view(np.uint32), rgba.cpu().numpy().view(np.uint32), var.cpu().numpy().view(np.uint32)
    assert (o[n:] == SENTINEL).all() and (r[n:] == SENTINEL).all() and (v[n:] == SENTINEL).all(), "words behind an output were written"
    if not in_place:   # the inputs are what they were
        assert np.array_equal(rec_t.cpu().numpy().view(np.uint32), records.view(np.uint32))
    assert np.array_equal(hv_t.cpu().numpy().view(np.uint32), halves.view(np.uint32)) and np.array_equal(al_t.cpu().numpy().view(np.uint32), albedo.view(np.uint32))
    if not rgba8:
        assert (r == SENTINEL).all()
    if not variance:
        assert (v == SENTINEL).all()
    return o[:n], v[:n], r[:n].view(np.uint8).reshape(n, 4)


def _check(got, want, what, rgba8=True, variance=True, nan_equal=False):
    """nan_equal: a word that is a NaN on both sides counts as equal whatever its other bits (a NaN the arithmetic generated has no
    specified sign or payload), and the bytes of a pixel with such a word are not compared.  "variance": in the variance words only,
    the records strict."""
    rec, var, rgba = got
    w = want["records"].view(np.uint32)
    if nan_equal:
        d_rec, n_rec = differing_words(rec, w)
        d_var, n_var = differing_words(var, want["variance"]) if variance else (0, 0)
        print(f"{what}: {n_rec} record and {n_var} variance words are NaNs of other bits on both sides")
        assert d_rec == 0, f"{what}: {d_rec} of {w.size} record words differ"
        assert d_var == 0, f"{what}: {d_var} variance words differ"
        assert n_rec == 0 or nan_equal != "variance", f"{what}: {n_rec} record words are NaNs of other bits"
        if rgba8:
            same = (rec == w).all(1)
            assert np.array_equal(rgba[same], want["rgba"][same]), f"{what}: {int((rgba[same] != want['rgba'][same]).sum())} bytes differ"
        return
    assert np.array_equal(rec, w), f"{what}: {int((rec != w).sum())} of {w.size} record words differ (first pixel {int(np.argwhere((rec != w).any(1))[0][0])})"
    if variance:
        assert np.array_equal(var, want["variance"].view(np.uint32)), f"{what}: {int((var != want['variance'].view(np.uint32)).sum())} variance words differ"
    if rgba8:
        assert np.array_equal(rgba, want["rgba"]), f"{what}: {int((rgba != want['rgba']).sum())} bytes differ"


# ---- 1: hand-made records against the yardstick ------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,iterations", ((1, 1, 1), (1, 1, 6), (3, 2, 5), (5, 5, 6), (37, 19, 5), (70, 41, 6), (130, 70, 6)))
def test_every_word_equals_the_yardstick(small_scene, W, H, iterations):
    prm = DenoiseParams(iterations=iterations)
    _check(_device_call(small_scene, W, H, True, True, prm), _yardstick(W, H, True, True, prm), f"{W}x{H} x{iterations}")


@pytest.mark.parametrize("W,H", ((37, 19), (130, 70)))
@pytest.mark.parametrize("use_halves,use_albedo", ((True, False), (False, True), (False, False)))
def test_with_and_without_halves_and_albedo(small_scene, W, H, use_halves, use_albedo):
    prm = DenoiseParams()
    _check(_device_call(small_scene, W, H, use_halves, use_albedo, prm), _yardstick(W, H, use_halves, use_albedo, prm), f"{W}x{H} halves={use_halves} albedo={use_albedo}")


@pytest.mark.parametrize("W,H", ((37, 19), (130, 70)))
def test_in_place_and_optional_outputs(small_scene, W, H):
    prm = DenoiseParams()
    want = _yardstick(W, H, True, True, prm)
    _check(_device_call(small_scene, W, H, True, True, prm, in_place=True), want, f"{W}x{H} in place")
    _check(_device_call(small_scene, W, H, True, True, prm, rgba8=False), want, f"{W}x{H} without rgba8_out", rgba8=False)
    _check(_device_call(small_scene, W, H, True, True, prm, variance=False), want, f"{W}x{H} without variance_out", variance=False)
    _check(_device_call(small_scene, W, H, True, True, prm, in_place=True, rgba8=False, variance=False), want, f"{W}x{H} out alone, in place", rgba8=False, variance=False)


@pytest.mark.parametrize("W,H", ((37, 19), (130, 70)))
@pytest.mark.parametrize("power", (0, 7))
def test_normal_power(small_scene, W, H, power):
    prm = DenoiseParams(normal_power_log2=power, sigma_depth=0.5, sigma_luminance=2.0)
    _check(_device_call(small_scene, W, H, True, False, prm), _yardstick(W, H, True, False, prm), f"{W}x{H} power {power}")


def test_every_form_of_the_pass_kernel_gives_the_same_bytes(small_scene, hip):
    """130x70 at 6 iterations: every pass gathered from global memory; every pass through an LDS tile of the frame where its halo fits
    (steps 1, 2, 4); every pass from step 2 on as one dense tile per residue class of the step's sub-lattice."""
    W, H = 130, 70
    prm = DenoiseParams(iterations=6)
    want = _yardstick(W, H, True, True, prm)
    try:
        for form in (hip.DENOISE_FORM_GATHER, hip.DENOISE_FORM_TILE, hip.DENOISE_FORM_LATTICE):
            hip.denoise_forms([form] * 6)
            _check(_device_call(small_scene, W, H, True, True, prm), want, f"form {form}")
        hip.denoise_forms([hip.DENOISE_FORM_LATTICE, hip.DENOISE_FORM_GATHER, hip.DENOISE_FORM_TILE, hip.DENOISE_FORM_LATTICE, hip.DENOISE_FORM_GATHER, hip.DENOISE_FORM_LATTICE])
        _check(_device_call(small_scene, 37, 19, False, True, prm), _yardstick(37, 19, False, True, prm), "mixed forms, 37x19")
    finally:
        hip.denoise_forms(None)


# ---- 2: the two forms, streams, pointers --------------------------------------------------------------------------------------------
def test_device_form_equals_host_form(small_scene):
    W, H = 130, 70
    prm = DenoiseParams()
    records, halves, albedo = random_frame(W, H)
    want = _yardstick(W, H, True, True, prm)
    host = small_scene.denoise_records(W, H, records, halves, albedo, prm, rgba8=True)
    dev = _device_call(small_scene, W, H, True, True, prm)
    assert np.array_equal(host["records"].view(np.uint32), dev[0]) and np.array_equal(host["variance"].view(np.uint32), dev[1]) and np.array_equal(host["rgba"], dev[2])
    _check((host["records"].view(np.uint32), host["variance"].view(np.uint32), host["rgba"]), want, "host form")
    in_place = small_scene.denoise_records(W, H, records, halves, None, prm, in_place=True, variance=False)
    assert np.array_equal(in_place["records"].view(np.uint32), _yardstick(W, H, True, False, prm)["records"].view(np.uint32))
    # gamma_correction reaches the bytes only
    g = small_scene.denoise_records(W, H, records, halves, albedo, DenoiseParams(gamma_correction=True), rgba8=True)
    assert np.array_equal(g["records"].view(np.uint32), host["records"].view(np.uint32)) and not np.array_equal(g["rgba"], host["rgba"])


def test_after_its_producer_on_a_non_null_stream(small_scene):
    import torch
    st = torch.cuda.Stream()
    prm = DenoiseParams()
    _check(_device_call(small_scene, 130, 70, True, True, prm, stream=st, produce=True), _yardstick(130, 70, True, True, prm), "behind its producer")
    _check(_device_call(small_scene, 37, 19, True, True, prm, stream=st, produce=True, in_place=True), _yardstick(37, 19, True, True, prm), "behind its producer, in place")


def test_pageable_host_memory_is_refused_by_name(small_scene, hip):
    import torch
    L = hip.lib()
    W, H = 37, 19
    n = W * H
    records, halves, albedo = random_frame(W, H)
    dev = dict(r=torch.from_numpy(records.copy()).cuda(), hv=torch.from_numpy(halves.copy()).cuda(), al=torch.from_numpy(albedo.copy()).cuda(),
               o=torch.full((n, 8), SENTINEL, dtype=torch.int32, device="cuda"), rg=torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda"),
               v=torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    host = dict(r=records.copy(), hv=halves.copy(), al=albedo.copy(), o=np.zeros((n, 8), F), rg=np.zeros((n, 4), np.uint8), v=np.zeros(n, F))
    prm = hip.denoise_default_params()
    for key, name in (("r", b"records_dev"), ("hv", b"halves_dev"), ("al", b"albedo_dev"), ("o", b"out_dev"), ("rg", b"rgba8_out_dev"), ("v", b"variance_out_dev")):
        p = {k: C.c_void_p(host[k].ctypes.data if k == key else dev[k].data_ptr()) for k in dev}
        rc = L.rr_denoise_records_device(small_scene._h, W, H, C.byref(prm), p["r"], p["hv"], p["al"], p["o"], p["rg"], p["v"], None)
        assert rc == -1 and name in L.rr_last_error(), (key, rc, L.rr_last_error())
    torch.cuda.synchronize()
    for k in ("o", "rg", "v"):
        assert (dev[k].cpu().numpy().view(np.uint32) == SENTINEL).all(), k


# ---- 3: the handle afterwards -------------------------------------------------------------------------------------------------------
def test_the_handle_renders_the_same_frame_before_and_after(hip):
    fs = _scene("spheres_room")
    cam = camera_for(fs, 50, 38).c_struct()
    cfg = _cfg("plain")
    prm = DenoiseParams()
    with hip.DeviceScene(fs, 0) as ds:
        first = ds.render(cam, cfg, aux=True); stats = ds.stats()
        _check(_device_call(ds, 130, 70, True, True, prm), _yardstick(130, 70, True, True, prm), "on a handle with a frame")
        assert ds.stats() == stats                      # nothing of a frame's statistics is touched
        second = ds.render(cam, cfg, aux=True)
        for k in ("rgba", "normal", "depth", "object_id"):
            assert np.array_equal(first[k], second[k], equal_nan=True), k


# ---- 4: end to end ------------------------------------------------------------------------------------------------------------------
def test_render_denoised_end_to_end(hip):
    """spheres_room, 50x38, 8 samples: Raytracing.render_denoised equals render_pixel_parts followed by the yardstick, bit for bit; its
    bytes are rr_render_pixels' byte rule on the filtered record; the torch form, with no host trip, gives the same."""
    import torch
    from rustray_amd import renderer
    from rustray_amd.renderer import Raytracing, _pack_records
    W, H = 50, 38
    fs = _scene("spheres_room")
    camera = camera_for(fs, W, H)
    rt = Raytracing(fs, camera, 0)
    try:
        rt.config = _cfg("plain", samples=8)
        base = rt.render_pixel_parts(n_parts=2)
        records, halves = _pack_records(base), _pack_records(base["parts"])
        want = atrous_denoise(records, halves, None, W, H)
        got = rt.render_denoised(rgba8=True)
        assert np.array_equal(got["noisy"].view(np.uint32), records.view(np.uint32))
        assert np.array_equal(got["records"].view(np.uint32), want["records"].view(np.uint32)), int((got["records"].view(np.uint32) != want["records"].view(np.uint32)).sum())
        assert np.array_equal(got["variance"].view(np.uint32), want["variance"].view(np.uint32))
        assert np.array_equal(got["rgba"], denoise.frame_bytes_linear(want["records"][:, 0:3]))
        assert np.array_equal(got["color"].view(np.uint32), want["records"][:, 0:3].view(np.uint32)) and np.array_equal(got["object_id"], base["object_id"])
        assert not np.array_equal(got["records"][:, 0:3], records[:, 0:3])       # the filter did something
        assert np.array_equal(got["records"][:, 3:].view(np.uint32), records[:, 3:].view(np.uint32))
        # the records route of denoise(): with an albedo of ones the demodulated colour is the colour
        again = rt.denoise(records, halves, np.ones((W * H, 3), F))
        assert np.array_equal(again["records"].view(np.uint32), want["records"].view(np.uint32))
        t = renderer.render_denoised_torch(rt.device_scene, camera.c_struct(), rt.config, rgba8=True)
        torch.cuda.synchronize()
        assert np.array_equal(t["records"].cpu().numpy().view(np.uint32), want["records"].view(np.uint32))
        assert np.array_equal(t["variance"].cpu().numpy().view(np.uint32), want["variance"].view(np.uint32))
        assert np.array_equal(t["rgba"].cpu().numpy(), got["rgba"]) and np.array_equal(t["halves"].cpu().numpy().view(np.uint32), halves.view(np.uint32))
    finally:
        rt.device_scene.close()
