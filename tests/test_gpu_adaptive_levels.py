"""rr_refine_sublist_device and rr_render_adaptive_levels: the noisy pixels of a frame refined level by level on the device.

1: the sublist kernels alone, on hand-made part records (no rendering), against rustray_amd/adaptive.py word for word; 2: the fused call
against the host loop Raytracing.render_adaptive_levels (spheres_room, 50 x 38, levels 6, 14, 30, threshold 0.1), against rr_render_pixels
at the three counts, against rr_render_adaptive for two levels, and its counters against the separate calls; 3: the device form; 4: the
handle afterwards; 5: caller tables."""
import ctypes as C

import numpy as np
import pytest

from rustray_amd import adaptive, capi
from tests.helpers import camera_for
from tests.test_gpu_adaptive_device import _parts_for, _random_parts
from tests.test_gpu_pixel_parts import ADAPTIVE_THRESHOLD, COUNTERS, FIELDS, H, N, SENTINEL, W, _bits, _cfg
from tests.test_gpu_shade_rays import _scene

pytestmark = pytest.mark.gpu

LEVELS = (6, 14, 30)
_cache = {}


@pytest.fixture(scope="module")
def small_scene(hip):
    with hip.DeviceScene(_scene("spheres_room"), 0) as ds:      # any small scene gives the handle
        yield ds


# ---- 1: the sublist kernels alone ------------------------------------------------------------------------------------------------
def _entries(n, seed):
    """n list entries with coordinates nobody interprets (any 32 bits), the second a duplicate of the first."""
    xy = np.random.default_rng(seed).integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    if n > 1:
        xy[1] = xy[0]
    return xy


def _check_sublist(ds, xy, count, parts, threshold, stream=None, produce=None, with_error=True):
    """One rr_refine_sublist_device call on the first `count` of the entries `xy` and on `parts` (len(xy), 2, 8) against adaptive.py; sentinels
    behind the list and the errors.  produce: a function that makes the device tensor of the parts on the current stream (the call then
    follows it without a synchronisation)."""
    import torch
    assert parts.shape == (len(xy), 2, 8) and count <= len(xy)
    want_err = adaptive.half_error(parts[:, :, 0:3])
    want_xy, want_taken = adaptive.refine_sublist(want_err, threshold, xy, count)
    room = (count + 63) // 64 * 64
    assert len(want_xy) <= room
    ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.device(0)
    with ctx:
        lst = torch.full((room + 5,), SENTINEL, dtype=torch.int32, device="cuda")
        err = torch.full((count + 3,), SENTINEL, dtype=torch.int32, device="cuda")
        src = torch.from_numpy(xy.view(np.int32)).cuda()
        t = produce() if produce is not None else torch.from_numpy(parts).cuda()
        if produce is None:
            torch.cuda.synchronize()
        taken = ds.refine_sublist_device(src.data_ptr(), count, t.data_ptr(), threshold, err.data_ptr() if with_error else None, lst.data_ptr(),
                                         stream.cuda_stream if stream is not None else None)
    torch.cuda.synchronize()
    got_l, got_e = lst.cpu().numpy().view(np.uint32), err.cpu().numpy().view(np.uint32)
    assert taken == want_taken, (taken, want_taken)
    assert np.array_equal(got_l[:len(want_xy)], want_xy), f"count {count}: the list differs in {int((got_l[:len(want_xy)] != want_xy).sum())} of {len(want_xy)} words"
    assert (got_l[len(want_xy):] == SENTINEL).all(), "words behind the padded length were written"
    if with_error:
        assert np.array_equal(got_e[:count], want_err[:count].view(np.uint32)) and (got_e[count:] == SENTINEL).all()
    else:
        assert (got_e == SENTINEL).all()
    assert np.array_equal(src.cpu().numpy().view(np.uint32), xy)                     # the input list is left as it was
    return want_taken, len(want_xy)


@pytest.mark.parametrize("count", (1, 63, 64, 65, 128))
def test_sublist_all_none_and_every_third(small_scene, count):
    xy = _entries(count, count)
    every = _parts_for(np.full(count, 0.5, np.float32))
    assert _check_sublist(small_scene, xy, count, every, 0.25) == (count, (count + 63) // 64 * 64)
    assert _check_sublist(small_scene, xy, count, every, 2.0) == (0, 0)              # nothing taken: no pad and no write
    third = np.where(np.arange(count) % 3 == 0, 0.5, 0.25).astype(np.float32)       # the others lie AT the threshold: not above it
    want = (count + 2) // 3
    assert _check_sublist(small_scene, xy, count, _parts_for(third), 0.25) == (want, (want + 63) // 64 * 64)


def test_sublist_never_looks_behind_count(small_scene):
    """A list with duplicates and with its own pad behind `count`; the pad's halves lie above the threshold, so a kernel that reads past
    `count` takes them.  Counts inside a wave, at its end and one past it."""
    for count in (10, 64, 65, 100):
        padded = (count + 63) // 64 * 64 + 64                                        # the pad, and a whole wave of it
        xy = _entries(padded, 40 + count)
        xy[3] = xy[7] = xy[0]
        xy[count:] = xy[count - 1]
        err = np.where(np.arange(padded) % 2 == 0, 0.5, 0.0).astype(np.float32)
        err[count - 1] = 0.0                                                         # the last entry itself is not taken: the pad repeats the last TAKEN one
        err[count:] = 0.5
        want = int((err[:count] > 0.25).sum())
        assert _check_sublist(small_scene, xy, count, _parts_for(err), 0.25) == (want, (want + 63) // 64 * 64)
        assert _check_sublist(small_scene, xy, count, _parts_for(err), 0.25, with_error=False)[0] == want      # error_out_dev == NULL


def test_sublist_of_random_halves(small_scene):
    parts = _random_parts(W, H, 15)
    c = parts[:, :, 0:3]
    assert np.isinf(c).any() and np.isnan(c).any() and (c > 1).any() and (c < 0).any()
    xy = _entries(N, 16)
    taken, padded = _check_sublist(small_scene, xy, N, parts, 0.1)
    assert 0 < taken < N
    assert _check_sublist(small_scene, xy, N, parts, -1.0) == (N, 1920)               # a negative threshold takes every entry, the non-finite ones too
    assert _check_sublist(small_scene, xy, N - 7, parts, -1.0) == (N - 7, 1920)


def test_sublist_crosses_the_scans_carry(small_scene):
    n = 264 * 264                                                                    # 1089 waves: more than one step of the scan
    rng = np.random.default_rng(18)
    err = np.where(rng.integers(0, 3, n) == 0, 0.5, 0.0).astype(np.float32)
    taken, padded = _check_sublist(small_scene, _entries(n, 19), n, _parts_for(err), 0.25)
    assert n // 4 < taken < n // 2


def test_sublist_of_nothing(small_scene, hip):
    import torch
    L = hip.lib()
    taken = C.c_uint32(77)
    assert L.rr_refine_sublist_device(small_scene._h, None, 0, None, C.c_float(0.1), None, None, C.byref(taken), None) == 0 and taken.value == 0
    lst = torch.full((64,), SENTINEL, dtype=torch.int32, device="cuda")
    parts = torch.from_numpy(_parts_for(np.full(64, 0.5, np.float32))).cuda()
    torch.cuda.synchronize()
    assert small_scene.refine_sublist_device(lst.data_ptr(), 0, parts.data_ptr(), 0.1, None, lst.data_ptr()) == 0    # (no overlap to refuse: nothing is read or written)
    torch.cuda.synchronize()
    assert (lst.cpu().numpy().view(np.uint32) == SENTINEL).all()


def test_sublist_after_its_producer_on_a_non_null_stream(small_scene):
    import torch
    parts = _random_parts(W, H, 26)
    st = torch.cuda.Stream()
    src = torch.from_numpy(parts).cuda()
    torch.cuda.synchronize()
    _check_sublist(small_scene, _entries(N, 27), N, parts, 0.1, stream=st, produce=src.clone)     # (a copy kernel on `st`; the call is enqueued behind it)


def test_sublist_refuses_pageable_host_memory_by_name(small_scene, hip):
    import torch
    L = hip.lib()
    parts = _random_parts(W, H, 28)
    xy = _entries(N, 29)
    lst = torch.full((1920,), SENTINEL, dtype=torch.int32, device="cuda")
    err = torch.full((N,), SENTINEL, dtype=torch.int32, device="cuda")
    src = torch.from_numpy(xy.view(np.int32)).cuda()
    t = torch.from_numpy(parts).cuda()
    torch.cuda.synchronize()
    taken = C.c_uint32(77)

    def call(s, p, e, l):
        return L.rr_refine_sublist_device(small_scene._h, C.c_void_p(s), N, C.c_void_p(p), C.c_float(0.1), C.c_void_p(e), C.c_void_p(l), C.byref(taken), None)
    host_l, host_e = np.zeros(1920, np.uint32), np.zeros(N, np.float32)
    assert call(xy.ctypes.data, t.data_ptr(), err.data_ptr(), lst.data_ptr()) == -1 and b"list_dev" in L.rr_last_error(), L.rr_last_error()
    assert call(src.data_ptr(), parts.ctypes.data, err.data_ptr(), lst.data_ptr()) == -1 and b"parts_dev" in L.rr_last_error(), L.rr_last_error()
    assert call(src.data_ptr(), t.data_ptr(), host_e.ctypes.data, lst.data_ptr()) == -1 and b"error_out_dev" in L.rr_last_error(), L.rr_last_error()
    assert call(src.data_ptr(), t.data_ptr(), err.data_ptr(), host_l.ctypes.data) == -1 and b"list_out_dev" in L.rr_last_error(), L.rr_last_error()
    assert call(src.data_ptr(), t.data_ptr(), err.data_ptr(), src.data_ptr()) == -1 and b"overlaps" in L.rr_last_error(), L.rr_last_error()
    torch.cuda.synchronize()
    assert (lst.cpu().numpy().view(np.uint32) == SENTINEL).all() and (err.cpu().numpy().view(np.uint32) == SENTINEL).all() and taken.value == 77


# ---- 2: the fused call against the host loop -------------------------------------------------------------------------------------
def _loop_with_stats(ds, cam, config, levels, threshold):
    """The host loop of Raytracing.render_adaptive_levels, call by call on `ds`, with the work counters of each call and each list's length."""
    stats, padded = [], []
    base = ds.render_pixel_parts(cam, _cfg(config, samples=levels[0]), None, n_parts=2)
    stats.append(ds.stats()); padded.append(N)
    xy, count = adaptive.refine_list(adaptive.half_error(base["parts"]["color"]), threshold, W, H)
    for s in levels[1:]:
        if not count:
            break
        fine = ds.render_pixel_parts(cam, _cfg(config, samples=s), xy, n_parts=2)
        stats.append(ds.stats()); padded.append(len(xy))
        xy, count = adaptive.refine_sublist(adaptive.half_error(fine["parts"]["color"]), threshold, xy, count)
    return stats, padded


def _fused(hip):
    """spheres_room, 50 x 38, the "plain" config, levels 6, 14, 30, on one handle: the host loop, the fused call at three thresholds (and with
    gamma_correction), rr_render_pixels at the three counts, two levels next to rr_render_adaptive, and the counters of the separate
    calls.  Computed once and left unchanged."""
    if "fused" not in _cache:
        from rustray_amd.renderer import Raytracing
        fs = _scene("spheres_room")
        camera = camera_for(fs, W, H)
        cam = camera.c_struct()
        c = dict(fs=fs, cam=cam)
        rt = Raytracing(fs, camera, 0)
        try:
            ds = rt.device_scene
            rt.config = _cfg("plain")
            c["host"] = rt.render_adaptive_levels(LEVELS, ADAPTIVE_THRESHOLD)
            c["on_device"] = rt.render_adaptive_levels_on_device(LEVELS, ADAPTIVE_THRESHOLD, rgba8=True)
            rt.config = _cfg("plain", gamma_correction=True)
            c["host_gamma"] = rt.render_adaptive_levels(LEVELS, ADAPTIVE_THRESHOLD)
            cfg = _cfg("plain", samples=1)          # config->samples is ignored
            c["fused"] = ds.render_adaptive_levels(cam, cfg, LEVELS, ADAPTIVE_THRESHOLD, rgba8=True); c["fused_stats"] = ds.stats()
            c["all"] = ds.render_adaptive_levels(cam, cfg, LEVELS, -1.0, rgba8=True); c["all_stats"] = ds.stats()
            c["none"] = ds.render_adaptive_levels(cam, cfg, LEVELS, 2.0, rgba8=True); c["none_stats"] = ds.stats()
            c["gamma"] = ds.render_adaptive_levels(cam, _cfg("plain", samples=1, gamma_correction=True), LEVELS, ADAPTIVE_THRESHOLD, rgba8=True)
            for s in LEVELS + (16,):
                c[s] = ds.render_pixels(cam, _cfg("plain", samples=s), None, rgba8=True)
                c[s, "gamma"] = ds.render_pixels(cam, _cfg("plain", samples=s, gamma_correction=True), None, rgba8=True)
            c["two"] = ds.render_adaptive_levels(cam, cfg, (6, 16), ADAPTIVE_THRESHOLD, rgba8=True)
            c["two_level_call"] = ds.render_adaptive(cam, cfg, 6, 16, ADAPTIVE_THRESHOLD, rgba8=True)
            c["parts16"] = ds.render_pixel_parts(cam, _cfg("plain", samples=16), None, n_parts=2)
            ds.render_adaptive(cam, cfg, 6, 30, ADAPTIVE_THRESHOLD); c["stats_6_30"] = ds.stats()
            c["loop_stats"], c["loop_padded"] = _loop_with_stats(ds, cam, "plain", LEVELS, ADAPTIVE_THRESHOLD)
        finally:
            rt.device_scene.close()
        _cache["fused"] = c
    return _cache["fused"]


def _same_frame(got, want, what, keys=FIELDS + ("samples", "error")):
    for k in keys:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k)
        assert np.array_equal(_bits(got[k]), _bits(want[k])), f"{what}: {k} differs in {int((_bits(got[k]) != _bits(want[k])).sum())} words"
    assert list(got["level_pixels"]) == list(want["level_pixels"]), (what, got["level_pixels"], want["level_pixels"])


def test_fused_call_equals_the_host_loop(hip):
    c = _fused(hip)
    print("level_pixels", c["fused"]["level_pixels"], "left above", int((c["fused"]["error"] > np.float32(ADAPTIVE_THRESHOLD)).sum()))
    for got, want, what in ((c["fused"], c["host"], "fused"), (c["on_device"], c["host"], "Raytracing"), (c["gamma"], c["host_gamma"], "gamma")):
        _same_frame(got, want, what)
        n0, n1, n2 = got["level_pixels"]
        assert n0 == N and N > n1 > n2 > 0, got["level_pixels"]
        for s in LEVELS:
            assert (got["samples"] == s).any(), f"no pixel ends at {s} samples"
        assert int((got["samples"] == 30).sum()) == n2 and int((got["samples"] >= 14).sum()) == n1
        assert set(np.unique(got["samples"])) == set(LEVELS)
        # every pixel ends below the threshold or at the top count
        assert ((got["error"] <= np.float32(ADAPTIVE_THRESHOLD)) | (got["samples"] == 30)).all()
        assert (got["error"][got["samples"] < 30] <= np.float32(ADAPTIVE_THRESHOLD)).all()


def test_every_record_is_render_pixels_record(hip):
    c = _fused(hip)
    for got, tag in ((c["fused"], None), (c["gamma"], "gamma")):
        assert got["rgba"].shape == (N, 4)
        for s in LEVELS:
            at = got["samples"] == s
            want = c[s] if tag is None else c[s, tag]
            assert 0 < at.sum() < N
            assert np.array_equal(got["rgba"][at], want["rgba"][at]), (s, "rgba")
            for k in FIELDS:
                assert np.array_equal(_bits(got[k])[at], _bits(want[k])[at]), (s, k)
    assert not np.array_equal(c["gamma"]["rgba"], c["fused"]["rgba"])          # the curve was applied
    for k in FIELDS + ("samples", "error"):
        assert np.array_equal(_bits(c["gamma"][k]), _bits(c["fused"][k])), k    # ... to the bytes only


def test_thresholds_minus_one_and_two(hip):
    c = _fused(hip)
    got = c["all"]                                                                # every pixel goes through all levels
    assert got["level_pixels"] == [N, N, N] and (got["samples"] == 30).all()
    for k in FIELDS + ("rgba",):
        assert np.array_equal(_bits(got[k]), _bits(c[30][k])), k
    assert c["all_stats"]["primary_rays"] == N * 6 + 1920 * 14 + 1920 * 30
    got = c["none"]                                                               # nothing is refined
    assert got["level_pixels"] == [N, 0, 0] and (got["samples"] == 6).all()
    for k in FIELDS + ("rgba",):
        assert np.array_equal(_bits(got[k]), _bits(c[6][k])), k
    assert np.array_equal(_bits(got["error"]), _bits(c["two_level_call"]["error"]))     # the base frame's error, as rr_render_adaptive reports it
    assert c["none_stats"]["primary_rays"] == N * 6


def test_two_levels_equal_rr_render_adaptive(hip):
    c = _fused(hip)
    got, want = c["two"], c["two_level_call"]
    for k in FIELDS + ("rgba", "samples"):
        assert np.array_equal(_bits(got[k]), _bits(want[k])), k
    assert got["level_pixels"] == [N, want["n_refined"]] and 0 < want["n_refined"] < N
    base = got["samples"] == 6
    assert np.array_equal(_bits(got["error"])[base], _bits(want["error"])[base])
    at16 = adaptive.half_error(c["parts16"]["parts"]["color"])
    assert np.array_equal(_bits(got["error"])[~base], _bits(at16)[~base])
    assert not np.array_equal(_bits(got["error"])[~base], _bits(want["error"])[~base])   # the residual error, not the one that had the pixel refined


def test_rays_are_the_sums_over_the_passes(hip):
    c = _fused(hip)
    stats, padded = c["loop_stats"], c["loop_padded"]
    assert len(stats) == 3 and padded[0] == N and all(p % 64 == 0 for p in padded[1:])
    assert [p >= n for p, n in zip(padded, c["fused"]["level_pixels"])] == [True] * 3
    for k in COUNTERS:
        assert c["fused_stats"][k] == sum(s[k] for s in stats), (k, c["fused_stats"][k], [s[k] for s in stats])
    want = sum(p * s for p, s in zip(padded, LEVELS))
    print("primary rays: level by level", c["fused_stats"]["primary_rays"], "two-level 6 -> 30", c["stats_6_30"]["primary_rays"])
    assert c["fused_stats"]["primary_rays"] == want
    assert c["fused_stats"]["primary_rays"] < c["stats_6_30"]["primary_rays"]


# ---- 3: the device form ----------------------------------------------------------------------------------------------------------
def test_device_form_equals_the_host_form(hip):
    import torch
    from rustray_amd import renderer
    c = _fused(hip)
    cam, cfg, want = c["cam"], _cfg("plain", samples=1), c["fused"]
    L = hip.lib()
    lv = (C.c_uint16 * 3)(*LEVELS)
    with hip.DeviceScene(c["fs"], 0) as ds:
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            got = renderer.render_adaptive_levels_torch(ds, cam, cfg, LEVELS, ADAPTIVE_THRESHOLD, rgba8=True)
        st.synchronize()
        rec = got["records"].cpu().numpy().view(np.uint32)
        assert got["level_pixels"] == want["level_pixels"] and rec.shape == (N, 8)
        assert np.array_equal(rec[:, 0:3], _bits(want["color"])) and np.array_equal(rec[:, 3], _bits(want["depth"]))
        assert np.array_equal(rec[:, 4:7], _bits(want["normal"])) and np.array_equal(rec[:, 7], want["object_id"])
        assert np.array_equal(got["samples"].cpu().numpy().astype(np.uint32), want["samples"])
        assert np.array_equal(_bits(got["error"].cpu().numpy()), _bits(want["error"])) and np.array_equal(got["rgba"].cpu().numpy(), want["rgba"])
        # sentinels behind every output, on a non-null stream
        out = torch.full((N + 2, 8), SENTINEL, dtype=torch.int32, device="cuda")
        rgba = torch.full((N + 2,), SENTINEL, dtype=torch.int32, device="cuda")
        smp = torch.full((N + 2,), 0x5a5a, dtype=torch.int16, device="cuda")
        err = torch.full((N + 2,), SENTINEL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        level_pixels = (C.c_uint32 * 4)(77, 77, 77, 77)

        def call(o=None, r=None, s=None, e=None):
            return L.rr_render_adaptive_levels_device(ds._h, C.byref(cam), C.byref(cfg), lv, 3, C.c_float(ADAPTIVE_THRESHOLD), None, C.c_void_p(o or out.data_ptr()),
                                                      C.c_void_p(r or rgba.data_ptr()), C.c_void_p(s or smp.data_ptr()), C.c_void_p(e or err.data_ptr()), level_pixels,
                                                      C.c_void_p(st.cuda_stream), None)
        # a host pointer is refused by argument name, with nothing written
        host = np.zeros((N, 8), np.float32)
        for kw, name in ((dict(o=host.ctypes.data), b"out_dev"), (dict(r=host.ctypes.data), b"rgba8_out_dev"), (dict(s=host.ctypes.data), b"samples_out_dev"),
                         (dict(e=host.ctypes.data), b"error_out_dev")):
            assert call(**kw) == -1 and name in L.rr_last_error(), L.rr_last_error()
        torch.cuda.synchronize()
        assert (out.cpu().numpy().view(np.uint32) == SENTINEL).all() and (rgba.cpu().numpy().view(np.uint32) == SENTINEL).all()
        assert (smp.cpu().numpy() == 0x5a5a).all() and (err.cpu().numpy().view(np.uint32) == SENTINEL).all() and list(level_pixels) == [77] * 4
        assert call() == 0 and list(level_pixels) == want["level_pixels"] + [77]
        st.synchronize()
        o, r, s, e = out.cpu().numpy().view(np.uint32), rgba.cpu().numpy().view(np.uint32), smp.cpu().numpy(), err.cpu().numpy().view(np.uint32)
        assert (o[N:] == SENTINEL).all() and (r[N:] == SENTINEL).all() and (s[N:] == 0x5a5a).all() and (e[N:] == SENTINEL).all()
        assert np.array_equal(o[:N], rec) and np.array_equal(r[:N].view(np.uint8).reshape(N, 4), want["rgba"])
        assert np.array_equal(s[:N].astype(np.uint32), want["samples"]) and np.array_equal(e[:N], _bits(want["error"]))
        # every optional output NULL: out_dev alone still equals the host form's
        only = torch.full((N + 2, 8), SENTINEL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert ds.render_adaptive_levels_device(cam, cfg, LEVELS, ADAPTIVE_THRESHOLD, only.data_ptr(), stream_ptr=st.cuda_stream) == want["level_pixels"]
        st.synchronize()
        o = only.cpu().numpy().view(np.uint32)
        assert np.array_equal(o[:N], rec) and (o[N:] == SENTINEL).all()
        assert ds.stats()["primary_rays"] == c["fused_stats"]["primary_rays"]


# ---- 4: the handle afterwards ----------------------------------------------------------------------------------------------------
def test_the_handle_afterwards(hip):
    c = _fused(hip)
    fs, cam = c["fs"], c["cam"]
    cfg = _cfg("plain")

    def frames_equal(a, b, what):
        for k in ("rgba", "normal", "depth", "object_id"):
            assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)

    edited = _scene("spheres_room")
    for m in edited.materials:
        m.base_color, m.specular_color = tuple(m.specular_color), tuple(m.base_color)
        m.reflectivity = 0.25
    with hip.DeviceScene(fs, 0) as ds:
        first = ds.render(cam, cfg, aux=True)
        got = ds.render_adaptive_levels(cam, cfg, LEVELS, ADAPTIVE_THRESHOLD, rgba8=True)
        second = ds.render(cam, cfg, aux=True)
        flag = C.c_int(1)
        with pytest.raises(hip.RustrayHipError) as ei:
            ds.render_adaptive_levels(cam, cfg, LEVELS, ADAPTIVE_THRESHOLD, cancel=flag)
        assert ei.value.code == -6
        third = ds.render(cam, cfg, aux=True)
        ds.update_materials(edited.materials)
        after_edit = ds.render_adaptive_levels(cam, cfg, LEVELS, ADAPTIVE_THRESHOLD, rgba8=True)
    with hip.DeviceScene(fs, 0) as fresh:
        want = fresh.render(cam, cfg, aux=True)
    with hip.DeviceScene(edited, 0) as fresh:
        want_edit = fresh.render_adaptive_levels(cam, cfg, LEVELS, ADAPTIVE_THRESHOLD, rgba8=True)
    frames_equal(first, second, "after a fused call")
    frames_equal(first, third, "after a cancelled fused call")
    frames_equal(first, want, "a fresh handle")
    _same_frame(got, c["fused"], "between two frames", FIELDS + ("samples", "error", "rgba"))
    _same_frame(after_edit, want_edit, "after rr_scene_update_materials", FIELDS + ("samples", "error", "rgba"))
    assert not np.array_equal(_bits(after_edit["color"]), _bits(got["color"]))


# ---- 5: caller tables ------------------------------------------------------------------------------------------------------------
def test_an_explicit_built_in_table_equals_null(hip):
    c = _fused(hip)
    table14, _ = capi.sample_table(14)
    with hip.DeviceScene(c["fs"], 0) as ds:
        got = ds.render_adaptive_levels(c["cam"], _cfg("plain", samples=1), LEVELS, ADAPTIVE_THRESHOLD, sample_xy_levels=[None, table14, None], rgba8=True)
        every = ds.render_adaptive_levels(c["cam"], _cfg("plain", samples=1), LEVELS, ADAPTIVE_THRESHOLD,
                                          sample_xy_levels=[capi.sample_table(s)[0] for s in LEVELS], rgba8=True)
    _same_frame(got, c["fused"], "level 1 under rr_sample_table(14)", FIELDS + ("samples", "error", "rgba"))
    _same_frame(every, c["fused"], "every level under its rr_sample_table", FIELDS + ("samples", "error", "rgba"))
