"""rr_refine_list_device and rr_render_adaptive: the noisy pixels of a frame found and refined on the device.

1: the list kernels alone, on hand-made part records (no rendering), against rustray_amd/adaptive.py word for word; 2: the fused call
against the host loop Raytracing.render_adaptive on the frame of tests/test_gpu_pixel_parts.py::test_render_adaptive (spheres_room, 50 x 38,
6 -> 16 samples, threshold 0.1), against rr_render_pixels at the two counts, and its counters against the two separate calls; 3: the
device form; 4: the handle afterwards."""
import ctypes as C

import numpy as np
import pytest

from rustray_amd import adaptive
from rustray_amd.flat import make_config
from tests.helpers import camera_for
from tests.test_gpu_pixel_parts import ADAPTIVE_THRESHOLD, COUNTERS, FIELDS, H, N, SENTINEL, W, _bits, _cfg, _index
from tests.test_gpu_shade_rays import _scene

pytestmark = pytest.mark.gpu

BASE, TOP = 6, 16
_cache = {}


# ---- 1: the list kernels alone ---------------------------------------------------------------------------------------------------
def _parts_for(err):
    """Part records (n, 2, 8) whose half_error is `err` (values in [0, 0.5], or NaN for a pixel without an estimate): A = (2 e, 0, 0), B = 0."""
    err = np.asarray(err, np.float32).reshape(-1)
    p = np.zeros((len(err), 2, 8), np.float32)
    p[:, 0, 0] = err * np.float32(2)
    p[:, :, 3:] = 7.0        # depth, normal, id: not looked at
    return p


def _check_list(ds, parts, w, h, threshold, stream=None, produce=None):
    """One rr_refine_list_device call on `parts` (n, 2, 8) against adaptive.py; sentinels behind both outputs.  produce: a function that makes the
    device tensor of the parts on the current stream (the call then follows it without a synchronisation)."""
    import torch
    n = w * h
    assert parts.shape == (n, 2, 8)
    want_err = adaptive.half_error(parts[:, :, 0:3])
    want_xy, want_count = adaptive.refine_list(want_err, threshold, w, h)
    cap = ds_capacity(w, h)
    assert cap == (n + 63) // 64 * 64 and len(want_xy) <= cap
    ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.device(0)
    with ctx:
        lst = torch.full((cap + 5,), SENTINEL, dtype=torch.int32, device="cuda")
        err = torch.full((n + 3,), SENTINEL, dtype=torch.int32, device="cuda")
        t = produce() if produce is not None else torch.from_numpy(parts).cuda()
        if produce is None:
            torch.cuda.synchronize()
        count = ds.refine_list_device(w, h, t.data_ptr(), threshold, err.data_ptr(), lst.data_ptr(), stream.cuda_stream if stream is not None else None)
    torch.cuda.synchronize()
    got_l, got_e = lst.cpu().numpy().view(np.uint32), err.cpu().numpy().view(np.uint32)
    assert count == want_count, (count, want_count)
    assert np.array_equal(got_l[:len(want_xy)], want_xy), f"{w}x{h}: the list differs in {int((got_l[:len(want_xy)] != want_xy).sum())} of {len(want_xy)} words"
    assert (got_l[len(want_xy):] == SENTINEL).all(), "words behind the padded length were written"
    assert np.array_equal(got_e[:n], want_err.view(np.uint32)) and (got_e[n:] == SENTINEL).all()
    return want_count, len(want_xy)


def ds_capacity(w, h):
    from rustray_amd import capi
    return capi.refine_list_capacity(w, h)


def _test_frame_20x12():
    w, h = 20, 12
    err = np.zeros((h, w), np.float32)
    for x, y in [(0, 0), (7, 7), (8, 0), (19, 3), (3, 8), (4, 8), (3, 9), (16, 11), (9, 1), (1, 9)]:
        err[y, x] = 0.5
    err[5, 5] = 0.25        # at the threshold: not above it
    err[6, 6] = np.nan      # a NaN half: error 0
    return w, h, err


def _random_parts(w, h, seed):
    rng = np.random.default_rng(seed)
    n = w * h
    p = rng.uniform(-0.5, 1.5, (n, 2, 8)).astype(np.float32)       # values above 1 and negative values
    special = np.array([np.inf, -np.inf, np.nan, 3.0, -2.0, 1.0, 0.0, -0.0], np.float32)
    at = rng.choice(n, n // 6, replace=False)
    p[at, rng.integers(0, 2, len(at)), rng.integers(0, 3, len(at))] = special[rng.integers(0, len(special), len(at))]
    return p


@pytest.fixture(scope="module")
def small_scene(hip):
    with hip.DeviceScene(_scene("spheres_room"), 0) as ds:      # any small scene gives the handle
        yield ds


def test_list_of_the_hand_made_frame(small_scene):
    w, h, err = _test_frame_20x12()
    parts = _parts_for(err)
    assert np.isnan(adaptive.half_error(parts[:, :, 0:3])).sum() == 0 and adaptive.half_error(parts[:, :, 0:3])[5 * w + 5] == np.float32(0.25)
    assert _check_list(small_scene, parts, w, h, 0.25) == (10, 64)


def test_list_counts_0_64_65(small_scene):
    w, h = 20, 12
    full = np.zeros((h, w), np.float32); full[:8, :8] = 0.5
    assert _check_list(small_scene, _parts_for(full), w, h, 0.25) == (64, 64)       # no pad
    assert _check_list(small_scene, _parts_for(full), w, h, 2.0) == (0, 0)          # nothing taken: no pad and no write
    full[0, 8] = 0.5
    assert _check_list(small_scene, _parts_for(full), w, h, 0.25) == (65, 128)      # a pad to 128


@pytest.mark.parametrize("w,h", ((1, 1), (9, 1), (8, 8)))
def test_list_of_small_frames_with_every_pixel_taken(small_scene, w, h):
    n = w * h
    assert _check_list(small_scene, _parts_for(np.full(n, 0.5, np.float32)), w, h, 0.25) == (n, 64)


def test_list_of_random_halves(small_scene):
    parts = _random_parts(W, H, 5)
    c = parts[:, :, 0:3]
    assert np.isinf(c).any() and np.isnan(c).any() and (c > 1).any() and (c < 0).any()
    count, padded = _check_list(small_scene, parts, W, H, 0.1)
    assert 0 < count < N
    assert _check_list(small_scene, parts, W, H, -1.0) == (N, 1920)                  # a negative threshold takes every pixel, the non-finite ones too


def test_list_crosses_the_scans_carry(small_scene):
    w = h = 264                                                                      # 33 x 33 = 1089 blocks: more than one step of the scan
    rng = np.random.default_rng(8)
    err = np.where(rng.integers(0, 3, w * h) == 0, 0.5, 0.0).astype(np.float32)
    count, padded = _check_list(small_scene, _parts_for(err), w, h, 0.25)
    assert w * h // 4 < count < w * h // 2


def test_list_after_its_producer_on_a_non_null_stream(small_scene):
    import torch
    parts = _random_parts(W, H, 6)
    st = torch.cuda.Stream()
    src = torch.from_numpy(parts).cuda()
    torch.cuda.synchronize()
    _check_list(small_scene, parts, W, H, 0.1, stream=st, produce=src.clone)     # (a copy kernel on `st`; the call is enqueued behind it)


def test_list_refuses_pageable_host_memory_by_name(small_scene, hip):
    import torch
    L = hip.lib()
    parts = _random_parts(W, H, 7)
    lst = torch.full((ds_capacity(W, H),), SENTINEL, dtype=torch.int32, device="cuda")
    err = torch.full((N,), SENTINEL, dtype=torch.int32, device="cuda")
    t = torch.from_numpy(parts).cuda()
    torch.cuda.synchronize()
    count = C.c_uint32(77)

    def call(p, e, l):
        return L.rr_refine_list_device(small_scene._h, W, H, C.c_void_p(p), 0.1, C.c_void_p(e), C.c_void_p(l), C.byref(count), None)
    host_l, host_e = np.zeros(ds_capacity(W, H), np.uint32), np.zeros(N, np.float32)
    assert call(parts.ctypes.data, err.data_ptr(), lst.data_ptr()) == -1 and b"parts_dev" in L.rr_last_error(), L.rr_last_error()
    assert call(t.data_ptr(), host_e.ctypes.data, lst.data_ptr()) == -1 and b"error_out_dev" in L.rr_last_error(), L.rr_last_error()
    assert call(t.data_ptr(), err.data_ptr(), host_l.ctypes.data) == -1 and b"list_out_dev" in L.rr_last_error(), L.rr_last_error()
    torch.cuda.synchronize()
    assert (lst.cpu().numpy().view(np.uint32) == SENTINEL).all() and (err.cpu().numpy().view(np.uint32) == SENTINEL).all() and count.value == 77


# ---- 2: the fused call against the host loop -------------------------------------------------------------------------------------
def _fused(hip):
    """spheres_room, 50 x 38, the "plain" config, 6 -> 16 samples, on one handle: the host loop, the fused call at three thresholds (and with
    gamma_correction), rr_render_pixels at both counts, and the counters of the two separate calls.  Computed once and left unchanged."""
    if "fused" not in _cache:
        from rustray_amd.renderer import Raytracing
        fs = _scene("spheres_room")
        camera = camera_for(fs, W, H)
        cam = camera.c_struct()
        c = dict(fs=fs, cam=cam)
        rt = Raytracing(fs, camera, 0)
        try:
            rt.config = _cfg("plain")
            ds = rt.device_scene
            c["host"] = rt.render_adaptive(BASE, TOP, ADAPTIVE_THRESHOLD)
            c["on_device"] = rt.render_adaptive_on_device(BASE, TOP, ADAPTIVE_THRESHOLD, rgba8=True)
            cfg = _cfg("plain", samples=1)          # config->samples is ignored
            c["fused"] = ds.render_adaptive(cam, cfg, BASE, TOP, ADAPTIVE_THRESHOLD, rgba8=True); c["fused_stats"] = ds.stats()
            c["all"] = ds.render_adaptive(cam, cfg, BASE, TOP, -1.0, rgba8=True); c["all_stats"] = ds.stats()
            c["none"] = ds.render_adaptive(cam, cfg, BASE, TOP, 2.0, rgba8=True); c["none_stats"] = ds.stats()
            c["gamma"] = ds.render_adaptive(cam, _cfg("plain", samples=1, gamma_correction=True), BASE, TOP, ADAPTIVE_THRESHOLD, rgba8=True)
            for s in (BASE, TOP):
                c[s] = ds.render_pixels(cam, _cfg("plain", samples=s), None, rgba8=True)
                c[s, "gamma"] = ds.render_pixels(cam, _cfg("plain", samples=s, gamma_correction=True), None, rgba8=True)
            xy, count = adaptive.refine_list(c["host"]["error"], ADAPTIVE_THRESHOLD, W, H)
            c["xy"], c["count"] = xy, count
            ds.render_pixel_parts(cam, _cfg("plain", samples=BASE), None, n_parts=2); c["stats_base"] = ds.stats()
            ds.render_pixels(cam, _cfg("plain", samples=TOP), xy); c["stats_fine"] = ds.stats()
        finally:
            rt.device_scene.close()
        _cache["fused"] = c
    return _cache["fused"]


def test_fused_call_equals_the_host_loop(hip):
    c = _fused(hip)
    for got in (c["fused"], c["on_device"]):
        for k in FIELDS + ("samples", "error"):
            assert got[k].shape == c["host"][k].shape and got[k].dtype == c["host"][k].dtype, k
            assert np.array_equal(_bits(got[k]), _bits(c["host"][k])), f"{k} differs in {int((_bits(got[k]) != _bits(c['host'][k])).sum())} words"
        assert got["n_refined"] == c["count"] and 0 < got["n_refined"] < N
        assert int((got["samples"] == TOP).sum()) == c["count"] and set(np.unique(got["samples"])) == {BASE, TOP}


def test_fused_bytes_are_render_pixels_bytes(hip):
    c = _fused(hip)
    for got, tag in ((c["fused"], None), (c["gamma"], "gamma")):
        refined = got["samples"] == TOP
        at6, at16 = (c[BASE], c[TOP]) if tag is None else (c[BASE, tag], c[TOP, tag])
        assert got["rgba"].shape == (N, 4) and 0 < refined.sum() < N
        assert np.array_equal(got["rgba"][refined], at16["rgba"][refined]) and np.array_equal(got["rgba"][~refined], at6["rgba"][~refined])
        for k in FIELDS:
            assert np.array_equal(_bits(got[k])[refined], _bits(at16[k])[refined]) and np.array_equal(_bits(got[k])[~refined], _bits(at6[k])[~refined]), k
    assert not np.array_equal(c["gamma"]["rgba"], c["fused"]["rgba"])          # the curve was applied
    for k in FIELDS:
        assert np.array_equal(_bits(c["gamma"][k]), _bits(c["fused"][k])), k    # ... to the bytes only


def test_every_pixel_and_no_pixel_refined(hip):
    c = _fused(hip)
    for got, want, n_ref, s in ((c["all"], c[TOP], N, TOP), (c["none"], c[BASE], 0, BASE)):
        assert got["n_refined"] == n_ref and (got["samples"] == s).all()
        for k in FIELDS + ("rgba",):
            assert np.array_equal(_bits(got[k]), _bits(want[k])), (s, k)
        assert np.array_equal(_bits(got["error"]), _bits(c["host"]["error"]))
    assert c["none_stats"]["primary_rays"] == N * BASE                            # the fine pass was skipped
    assert c["all_stats"]["primary_rays"] == N * BASE + 1920 * TOP


def test_stats_are_the_sums_over_the_two_passes(hip):
    c = _fused(hip)
    padded = len(c["xy"])
    assert padded % 64 == 0 and padded >= c["count"]
    for k in COUNTERS:
        assert c["fused_stats"][k] == c["stats_base"][k] + c["stats_fine"][k], (k, c["fused_stats"][k], c["stats_base"][k], c["stats_fine"][k])
    assert c["fused_stats"]["primary_rays"] == N * BASE + padded * TOP


# ---- 3: the device form ----------------------------------------------------------------------------------------------------------
def test_device_form_equals_the_host_form(hip):
    import torch
    from rustray_amd import renderer
    c = _fused(hip)
    cam, cfg, want = c["cam"], _cfg("plain", samples=1), c["fused"]
    L = hip.lib()
    with hip.DeviceScene(c["fs"], 0) as ds:
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            got = renderer.render_adaptive_torch(ds, cam, cfg, BASE, TOP, ADAPTIVE_THRESHOLD, rgba8=True)
        st.synchronize()
        rec = got["records"].cpu().numpy().view(np.uint32)
        assert got["n_refined"] == want["n_refined"] and rec.shape == (N, 8)
        assert np.array_equal(rec[:, 0:3], _bits(want["color"])) and np.array_equal(rec[:, 3], _bits(want["depth"]))
        assert np.array_equal(rec[:, 4:7], _bits(want["normal"])) and np.array_equal(rec[:, 7], want["object_id"])
        assert np.array_equal(got["samples"].cpu().numpy().astype(np.uint32), want["samples"])
        assert np.array_equal(_bits(got["error"].cpu().numpy()), _bits(want["error"])) and np.array_equal(got["rgba"].cpu().numpy(), want["rgba"])
        assert got["color"].data_ptr() == got["records"].data_ptr()
        # sentinels behind every output, on a non-null stream
        out = torch.full((N + 2, 8), SENTINEL, dtype=torch.int32, device="cuda")
        rgba = torch.full((N + 2,), SENTINEL, dtype=torch.int32, device="cuda")
        smp = torch.full((N + 2,), 0x5a5a, dtype=torch.int16, device="cuda")
        err = torch.full((N + 2,), SENTINEL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        count = C.c_uint32(77)

        def call(o=None, r=None, s=None, e=None):
            return L.rr_render_adaptive_device(ds._h, C.byref(cam), C.byref(cfg), BASE, TOP, ADAPTIVE_THRESHOLD, None, None, C.c_void_p(o or out.data_ptr()),
                                               C.c_void_p(r or rgba.data_ptr()), C.c_void_p(s or smp.data_ptr()), C.c_void_p(e or err.data_ptr()), C.byref(count),
                                               C.c_void_p(st.cuda_stream), None)
        # a host pointer is refused by argument name, with nothing written
        host = np.zeros((N, 8), np.float32)
        for kw, name in ((dict(o=host.ctypes.data), b"out_dev"), (dict(r=host.ctypes.data), b"rgba8_out_dev"), (dict(s=host.ctypes.data), b"samples_out_dev"),
                         (dict(e=host.ctypes.data), b"error_out_dev")):
            assert call(**kw) == -1 and name in L.rr_last_error(), L.rr_last_error()
        torch.cuda.synchronize()
        assert (out.cpu().numpy().view(np.uint32) == SENTINEL).all() and (rgba.cpu().numpy().view(np.uint32) == SENTINEL).all()
        assert (smp.cpu().numpy() == 0x5a5a).all() and (err.cpu().numpy().view(np.uint32) == SENTINEL).all() and count.value == 77
        assert call() == 0 and count.value == want["n_refined"]
        st.synchronize()
        o, r, s, e = out.cpu().numpy().view(np.uint32), rgba.cpu().numpy().view(np.uint32), smp.cpu().numpy(), err.cpu().numpy().view(np.uint32)
        assert (o[N:] == SENTINEL).all() and (r[N:] == SENTINEL).all() and (s[N:] == 0x5a5a).all() and (e[N:] == SENTINEL).all()
        assert np.array_equal(o[:N], rec) and np.array_equal(r[:N].view(np.uint8).reshape(N, 4), want["rgba"])
        assert np.array_equal(s[:N].astype(np.uint32), want["samples"]) and np.array_equal(e[:N], _bits(want["error"]))
        # every optional output NULL: out_dev alone still equals the host form's
        only = torch.full((N + 2, 8), SENTINEL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert ds.render_adaptive_device(cam, cfg, BASE, TOP, ADAPTIVE_THRESHOLD, only.data_ptr(), stream_ptr=st.cuda_stream) == want["n_refined"]
        st.synchronize()
        o = only.cpu().numpy().view(np.uint32)
        assert np.array_equal(o[:N], rec) and (o[N:] == SENTINEL).all()


# ---- 4: the handle afterwards ----------------------------------------------------------------------------------------------------
def test_the_handle_afterwards(hip):
    c = _fused(hip)
    fs, cam = c["fs"], c["cam"]
    cfg = _cfg("plain")

    def frames_equal(a, b, what):
        for k in ("rgba", "normal", "depth", "object_id"):
            assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)

    def same(a, b, what):
        for k in FIELDS + ("samples", "error", "rgba"):
            assert np.array_equal(_bits(a[k]), _bits(b[k])), (what, k)
        assert a["n_refined"] == b["n_refined"]

    edited = _scene("spheres_room")
    for m in edited.materials:
        m.base_color, m.specular_color = tuple(m.specular_color), tuple(m.base_color)
        m.reflectivity = 0.25
    with hip.DeviceScene(fs, 0) as ds:
        first = ds.render(cam, cfg, aux=True)
        got = ds.render_adaptive(cam, cfg, BASE, TOP, ADAPTIVE_THRESHOLD, rgba8=True)
        second = ds.render(cam, cfg, aux=True)
        flag = C.c_int(1)
        with pytest.raises(hip.RustrayHipError) as ei:
            ds.render_adaptive(cam, cfg, BASE, TOP, ADAPTIVE_THRESHOLD, cancel=flag)
        assert ei.value.code == -6
        third = ds.render(cam, cfg, aux=True)
        ds.update_materials(edited.materials)
        after_edit = ds.render_adaptive(cam, cfg, BASE, TOP, ADAPTIVE_THRESHOLD, rgba8=True)
    with hip.DeviceScene(fs, 0) as fresh:
        want = fresh.render(cam, cfg, aux=True)
    with hip.DeviceScene(edited, 0) as fresh:
        want_edit = fresh.render_adaptive(cam, cfg, BASE, TOP, ADAPTIVE_THRESHOLD, rgba8=True)
    frames_equal(first, second, "after a fused call")
    frames_equal(first, third, "after a cancelled fused call")
    frames_equal(first, want, "a fresh handle")
    same(got, c["fused"], "between two frames")
    same(after_edit, want_edit, "after rr_scene_update_materials")
    assert not np.array_equal(_bits(after_edit["color"]), _bits(got["color"]))
