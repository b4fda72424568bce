"""rr_render_pixel_prefix and rr_render_adaptive_prefix: the first samples of a frame as records, and a frame refined level by level whose
pixels keep their samples.

spheres_room at 50 x 38 (partial 8x8 blocks), monte_carlo.  1: the prefix of the 30-sample frame -- the whole prefix against
rr_render_pixels and rr_render_pixel_parts, shorter ones against the oracle's samples_used means, lists, batches, the device form, the
handle afterwards; 2: the fused call on the ladders (6, 14, 30) and (8, 16, 32) against the host loop Raytracing.render_adaptive_prefix,
against rr_render_pixel_prefix at every count, at thresholds -1, 2 and one in the middle, its counters, a list that crosses the scan's
carry, the device form, a cancel, an edit."""
import ctypes as C

import numpy as np
import pytest

from rustray_amd import adaptive
from tests.helpers import BAND_EPS_ABS, BAND_EPS_REL, D6_CLAMP, U32, camera_for, depth_check, normal_check
from tests.test_gpu_pixel_parts import COUNTERS, FIELDS, H, N, SENTINEL, W, _bits, _cfg, _pick, _same, _same_parts
from tests.test_gpu_render_pixels import _all_pixels_shuffled, _index
from tests.test_gpu_shade_rays import _scene

pytestmark = pytest.mark.gpu

S = 30
LADDERS = {30: (6, 14, 30), 32: (8, 16, 32)}
ORACLE_COUNTS = (2, 6, 14, 16)
_cache = {}


def _base(hip):
    """The scene, the camera, and on one handle rr_render_pixels and rr_render_pixel_parts (K = 2) of the 30-sample frame, with and without
    gamma, and the prefixes the tests below compare with.  Computed once and left unchanged."""
    if "base" not in _cache:
        fs = _scene("spheres_room")
        cam = camera_for(fs, W, H).c_struct()
        c = dict(fs=fs, cam=cam, prefix={}, halves={}, stats={})
        with hip.DeviceScene(fs, 0) as ds:
            for gamma in (False, True):
                cfg = _cfg("plain", samples=S, gamma_correction=gamma)
                c["pixels", gamma] = ds.render_pixels(cam, cfg, None, rgba8=True)
                c["parts", gamma] = ds.render_pixel_parts(cam, cfg, None, n_parts=2)
                c["whole", gamma] = ds.render_pixel_prefix(cam, cfg, None, samples_used=S, rgba8=True); c["whole_stats", gamma] = ds.stats()
                c["whole_halves", gamma] = ds.render_pixel_prefix(cam, cfg, None, samples_used=S, halves=True, rgba8=True)
            cfg = _cfg("plain", samples=S)
            for k in sorted(set(ORACLE_COUNTS + LADDERS[30] + (1, 29))):
                c["prefix"][k] = ds.render_pixel_prefix(cam, cfg, None, samples_used=k, rgba8=True); c["stats"][k] = ds.stats()
                if k % 2 == 0:
                    c["halves"][k] = ds.render_pixel_prefix(cam, cfg, None, samples_used=k, halves=True, rgba8=True)
        _cache["base"] = c
    return _cache["base"]


# ---- 1: the prefix ---------------------------------------------------------------------------------------------------------------
def test_the_whole_prefix_is_the_frame(hip):
    c = _base(hip)
    for gamma in (False, True):
        _same(c["whole", gamma], c["pixels", gamma], f"samples_used = S, gamma {gamma}", FIELDS + ("rgba",))
        _same(c["whole_halves", gamma], c["pixels", gamma], f"samples_used = S with halves, gamma {gamma}", FIELDS + ("rgba",))
        _same_parts(c["whole_halves", gamma], c["parts", gamma], f"halves at samples_used = S, gamma {gamma}")
        assert c["whole_stats", gamma]["primary_rays"] == N * S
    assert not np.array_equal(c["whole", True]["rgba"], c["whole", False]["rgba"])          # the curve was applied ...
    _same(c["whole", True], c["whole", False], "gamma", FIELDS)                             # ... to the bytes only


@pytest.mark.parametrize("k", ORACLE_COUNTS)
def test_prefix_against_the_oracles_samples_used_means(hip, oracle, k):
    """As tests/test_gpu_render_pixels.py judges a record against the oracle's frame, here against its samples_used = k means: ids equal
    (the id of sample k - 1), every colour channel inside the band around the float64 mean, depth and normal through the helpers."""
    c = _base(hip)
    cfg = _cfg("plain", samples=S)
    ref = oracle.render(c["fs"].c_struct(), c["cam"], cfg, want_means=True, want_counters=True, n_threads=16, samples_used=k)
    got = c["prefix"][k]
    m = ref["mean_rgb"].reshape(N, 3)
    assert np.isfinite(m).all() and not (ref["max_abs_rgb"] > D6_CLAMP).any()
    assert np.array_equal(got["object_id"], ref["object_id"].reshape(N))
    e = BAND_EPS_REL * np.abs(m) + BAND_EPS_ABS + 4 * U32 * np.abs(m)
    err = np.abs(got["color"].astype(np.float64) - m)
    worst = float((err / e).max())
    print(f"render_pixel_prefix samples_used {k}: worst |color - m| / e = {worst:.4f}")
    assert (err <= e).all(), f"samples_used {k}: {int((err > e).sum())} channels outside, worst |color - m| / e = {worst:.4f}"
    dc = depth_check(got["depth"], ref["depth"].reshape(N), ref["mean_depth"].reshape(N))
    nc = normal_check(got["normal"], ref["mean_normal"].reshape(N, 3))
    assert dc["n_depth_outside"] == 0 and nc["n_normal_outside"] == 0, (dc, nc, worst)
    assert c["stats"][k]["primary_rays"] == ref["counters"]["rays_primary"] == N * k
    assert c["stats"][k]["secondary_rays"] == ref["counters"]["rays_secondary"] and c["stats"][k]["shaded_hits"] == ref["counters"]["shaded_hits"]


def test_halves_are_the_interleaved_halves_of_the_prefix(hip):
    """With halves the full record is the one without them, and the halves' integer sums add up to it: mean = (A + B) / 2 to the rounding
    of the three divisions (|A|, |B| and |mean| times 2^-23 at most, plus the 2^-24 quantum of a sum)."""
    c = _base(hip)
    for k, hv in c["halves"].items():
        _same(hv, c["prefix"][k], f"samples_used {k}", FIELDS + ("rgba",))
        a, b = hv["parts"]["color"][:, 0].astype(np.float64), hv["parts"]["color"][:, 1].astype(np.float64)
        full = hv["color"].astype(np.float64)
        tol = 2.0 ** -22 * (np.abs(a) + np.abs(b) + np.abs(full)) + 2.0 ** -23
        assert (np.abs((a + b) / 2 - full) <= tol).all(), k
        assert np.array_equal(hv["parts"]["object_id"][:, 0], hv["object_id"]) and np.array_equal(hv["parts"]["object_id"][:, 1], hv["object_id"])
    assert not np.array_equal(_bits(c["prefix"][14]["color"]), _bits(c["prefix"][16]["color"]))
    # odd counts have no halves but are prefixes like any other
    assert c["stats"][1]["primary_rays"] == N and c["stats"][29]["primary_rays"] == N * 29


def test_lists_equal_the_whole_frame_record_by_record(hip):
    c = _base(hip)
    cfg = _cfg("plain", samples=S)
    perm = _all_pixels_shuffled()
    lists = {f"prefix {n}": perm[:n] for n in (1, 63, 64, 65)}
    lists["twice"] = np.repeat(perm[:300], 2)
    with hip.DeviceScene(c["fs"], 0) as ds:
        for what, xy in lists.items():
            for k in (14, 16):
                got = ds.render_pixel_prefix(c["cam"], cfg, xy, samples_used=k, halves=True, rgba8=True)
                assert ds.stats()["primary_rays"] == len(xy) * k, (what, k)
                want = _pick(c["halves"][k], _index(xy)); want["rgba"] = c["halves"][k]["rgba"][_index(xy)]
                _same(got, want, f"{what} at {k}", FIELDS + ("rgba",)); _same(got["parts"], want["parts"], f"{what} at {k} (halves)")
            got = ds.render_pixel_prefix(c["cam"], cfg, xy, samples_used=29, rgba8=True)
            _same(got, {f: c["prefix"][29][f][_index(xy)] for f in FIELDS + ("rgba",)}, f"{what} at 29", FIELDS + ("rgba",))
        with pytest.raises(hip.RustrayHipError) as ei:
            ds.render_pixel_prefix(c["cam"], cfg, np.array([W | (3 << 16)], np.uint32), samples_used=6)
        assert ei.value.code == -1 and b"pixel_xy[0]" in hip.lib().rr_last_error()


def test_several_batches_give_the_same_bits(hip):
    c = _base(hip)
    cfg = _cfg("plain", samples=S)
    with hip.DeviceScene(c["fs"], 0) as ds:
        ds.set_tuning(queue_budget_bytes=56 * (3 * 9000 + 2 * 256 * 5))
        for k in (14, 16):
            got = ds.render_pixel_prefix(c["cam"], cfg, None, samples_used=k, halves=True, rgba8=True)
            st = ds.stats()
            assert st["batches"] > 1 and st["primary_rays"] == N * k, st
            _same(got, c["halves"][k], f"{k} samples in {st['batches']} batches", FIELDS + ("rgba",)); _same(got["parts"], c["halves"][k]["parts"], "halves")
        got = ds.render_pixel_prefix(c["cam"], cfg, None, samples_used=29, rgba8=True)
        assert ds.stats()["batches"] > 1
        _same(got, c["prefix"][29], "29 samples in batches", FIELDS + ("rgba",))


def test_prefix_device_form_on_a_stream(hip):
    import torch
    c = _base(hip)
    cfg = _cfg("plain", samples=S)
    want = c["halves"][14]
    xy = _all_pixels_shuffled()[:65]
    with hip.DeviceScene(c["fs"], 0) as ds:
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            out = torch.full((N + 2, 8), SENTINEL, dtype=torch.int32, device="cuda")
            hv = torch.full((2 * N + 2, 8), SENTINEL, dtype=torch.int32, device="cuda")
            rgba = torch.full((N + 2,), SENTINEL, dtype=torch.int32, device="cuda")
            lst = torch.from_numpy(xy.view(np.int32)).cuda()
        torch.cuda.synchronize()
        host = np.zeros((N, 8), np.float32)
        L = hip.lib()
        for kw, name in ((dict(out_ptr=host.ctypes.data), b"out_dev"), (dict(halves_ptr=host.ctypes.data), b"halves_out_dev"), (dict(rgba8_ptr=host.ctypes.data), b"rgba8_out_dev")):
            args = dict(out_ptr=out.data_ptr(), halves_ptr=hv.data_ptr(), rgba8_ptr=rgba.data_ptr()); args.update(kw)
            with pytest.raises(hip.RustrayHipError):
                ds.render_pixel_prefix_device(c["cam"], cfg, None, N, 14, stream_ptr=st.cuda_stream, **args)
            assert name in L.rr_last_error(), L.rr_last_error()
        torch.cuda.synchronize()
        assert (out.cpu().numpy().view(np.uint32) == SENTINEL).all() and (hv.cpu().numpy().view(np.uint32) == SENTINEL).all()
        ds.render_pixel_prefix_device(c["cam"], cfg, None, N, 14, out.data_ptr(), hv.data_ptr(), rgba.data_ptr(), stream_ptr=st.cuda_stream)
        st.synchronize()
        o, p, r = out.cpu().numpy().view(np.uint32), hv.cpu().numpy().view(np.uint32), rgba.cpu().numpy().view(np.uint32)
        assert (o[N:] == SENTINEL).all() and (p[2 * N:] == SENTINEL).all() and (r[N:] == SENTINEL).all()
        assert np.array_equal(o[:N, 0:3], _bits(want["color"])) and np.array_equal(o[:N, 3], _bits(want["depth"]))
        assert np.array_equal(o[:N, 4:7], _bits(want["normal"])) and np.array_equal(o[:N, 7], want["object_id"])
        assert np.array_equal(p[:2 * N].reshape(N, 2, 8)[:, :, 0:3], _bits(want["parts"]["color"]))
        assert np.array_equal(r[:N].view(np.uint8).reshape(N, 4), want["rgba"])
        # a list, without halves and bytes
        only = torch.full((65 + 2, 8), SENTINEL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ds.render_pixel_prefix_device(c["cam"], cfg, lst.data_ptr(), 65, 29, only.data_ptr(), stream_ptr=st.cuda_stream)
        st.synchronize()
        o = only.cpu().numpy().view(np.uint32)
        assert (o[65:] == SENTINEL).all() and np.array_equal(o[:65, 0:3], _bits(c["prefix"][29]["color"][_index(xy)]))
        assert ds.stats()["primary_rays"] == 65 * 29


def test_frames_before_and_after_a_prefix(hip):
    c = _base(hip)
    cfg, cfg6 = _cfg("plain", samples=S), _cfg("plain")
    with hip.DeviceScene(c["fs"], 0) as ds:
        first = ds.render(c["cam"], cfg6, aux=True)
        a = ds.render_pixel_prefix(c["cam"], cfg, None, samples_used=14, halves=True, rgba8=True)
        second = ds.render(c["cam"], cfg6, aux=True)
        full = ds.render_pixels(c["cam"], cfg, None, rgba8=True)
        flag = C.c_int(1)
        with pytest.raises(hip.RustrayHipError) as ei:
            ds.render_pixel_prefix(c["cam"], cfg, None, samples_used=14, cancel=flag)
        assert ei.value.code == -6
        third = ds.render(c["cam"], cfg6, aux=True)
    for f in ("rgba", "normal", "depth", "object_id"):
        assert np.array_equal(first[f], second[f], equal_nan=True) and np.array_equal(first[f], third[f], equal_nan=True), f
    _same(a, c["halves"][14], "between two frames", FIELDS + ("rgba",))
    _same(full, c["pixels", False], "rr_render_pixels after a prefix of the same frame", FIELDS + ("rgba",))


# ---- 2: the fused ladder ---------------------------------------------------------------------------------------------------------
def _middle_threshold(rt, ladder):
    """A threshold, chosen on the HOST LOOP, under which every level is non-empty and at least one list length is no multiple of 64: the
    median of the first prefix's errors, lowered until both hold."""
    base = rt.render_pixel_prefix(ladder[0], halves=True)
    e0 = np.sort(adaptive.half_error(base["parts"]["color"]))
    for q in (0.8, 0.7, 0.6, 0.5, 0.4, 0.3, 0.2):
        thr = float(e0[int(q * N)])
        host = rt.render_adaptive_prefix(ladder, thr)
        lp = host["level_pixels"]
        if all(n > 0 for n in lp) and any(n % 64 for n in lp[1:]) and lp[-1] < lp[1] < N:
            return thr, host
    raise AssertionError("no threshold with every level non-empty")


def _fused(hip, top):
    """One ladder on one handle: the host loop (the yardstick), the fused call at three thresholds and under gamma, rr_render_pixel_prefix at
    every count, rr_render_pixels of the whole frame.  Computed once and left unchanged."""
    key = ("fused", top)
    if key not in _cache:
        from rustray_amd.renderer import Raytracing
        ladder = LADDERS[top]
        fs = _scene("spheres_room")
        camera = camera_for(fs, W, H)
        cam = camera.c_struct()
        c = dict(fs=fs, cam=cam, ladder=ladder, prefix={}, prefix_gamma={})
        rt = Raytracing(fs, camera, 0)
        try:
            ds = rt.device_scene
            rt.config = cfg = _cfg("plain", samples=top)
            c["threshold"], c["host"] = _middle_threshold(rt, ladder)
            thr = c["threshold"]
            c["on_device"] = rt.render_adaptive_prefix_on_device(ladder, thr, rgba8=True)
            c["fused"] = ds.render_adaptive_prefix(cam, cfg, ladder, thr, rgba8=True); c["fused_stats"] = ds.stats()
            c["all"] = ds.render_adaptive_prefix(cam, cfg, ladder, -1.0, rgba8=True); c["all_stats"] = ds.stats()
            c["none"] = ds.render_adaptive_prefix(cam, cfg, ladder, 2.0, rgba8=True); c["none_stats"] = ds.stats()
            c["host_none"] = rt.render_adaptive_prefix(ladder, 2.0)
            c["host_all"] = rt.render_adaptive_prefix(ladder, -1.0)
            cfg_g = _cfg("plain", samples=top, gamma_correction=True)
            c["gamma"] = ds.render_adaptive_prefix(cam, cfg_g, ladder, thr, rgba8=True)
            for k in ladder:
                c["prefix"][k] = ds.render_pixel_prefix(cam, cfg, None, samples_used=k, rgba8=True)
                c["prefix_gamma"][k] = ds.render_pixel_prefix(cam, cfg_g, None, samples_used=k, rgba8=True)
            c["pixels"] = ds.render_pixels(cam, cfg, None, rgba8=True)
        finally:
            rt.device_scene.close()
        _cache[key] = c
    return _cache[key]


def _same_frame(got, want, what, keys=FIELDS + ("samples", "error")):
    for k in keys:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k)
        assert np.array_equal(_bits(got[k]), _bits(want[k])), f"{what}: {k} differs in {int((_bits(got[k]) != _bits(want[k])).sum())} words"
    assert list(got["level_pixels"]) == list(want["level_pixels"]), (what, got["level_pixels"], want["level_pixels"])


@pytest.mark.parametrize("top", (30, 32))
def test_fused_call_equals_the_host_loop(hip, top):
    c = _fused(hip, top)
    thr, ladder = np.float32(c["threshold"]), c["ladder"]
    print("ladder", ladder, "threshold", c["threshold"], "level_pixels", c["fused"]["level_pixels"], "padded", c["host"]["padded"], "primary_rays",
          c["fused_stats"]["primary_rays"], "left above", int((c["fused"]["error"] > thr).sum()))
    for got, what in ((c["fused"], "fused"), (c["on_device"], "Raytracing"), (c["gamma"], "gamma")):
        _same_frame(got, c["host"], what)
        lp = got["level_pixels"]
        assert lp[0] == N and all(a >= b for a, b in zip(lp, lp[1:])) and lp[-1] > 0 and any(n % 64 for n in lp[1:]), lp
        assert set(np.unique(got["samples"])) == set(ladder)
        for l, k in enumerate(ladder):
            assert int((got["samples"] >= k).sum()) == lp[l]
        assert ((got["error"] <= thr) | (got["samples"] == top)).all()
    _same_frame(c["none"], c["host_none"], "threshold 2")
    _same_frame(c["all"], c["host_all"], "threshold -1")


@pytest.mark.parametrize("top", (30, 32))
def test_every_record_is_the_prefix_record_at_its_count(hip, top):
    c = _fused(hip, top)
    for got, prefix in ((c["fused"], c["prefix"]), (c["gamma"], c["prefix_gamma"])):
        for k in c["ladder"]:
            at = got["samples"] == k
            assert 0 < at.sum() < N
            for f in FIELDS + ("rgba",):
                assert np.array_equal(_bits(got[f])[at], _bits(prefix[k][f])[at]), (k, f)
    assert not np.array_equal(c["gamma"]["rgba"], c["fused"]["rgba"])
    for f in FIELDS + ("samples", "error"):
        assert np.array_equal(_bits(c["gamma"][f]), _bits(c["fused"][f])), f


@pytest.mark.parametrize("top", (30, 32))
def test_thresholds_minus_one_and_two(hip, top):
    """Threshold -1: every pixel climbs to the top, through continued accumulation, every compaction and the pad, and ends as
    rr_render_pixels' pixel of the whole frame.  Threshold 2: nobody climbs."""
    c = _fused(hip, top)
    ladder = c["ladder"]
    got = c["all"]
    assert got["level_pixels"] == [N] * 3 and (got["samples"] == top).all()
    for f in FIELDS + ("rgba",):
        assert np.array_equal(_bits(got[f]), _bits(c["pixels"][f])), f
    assert c["all_stats"]["primary_rays"] == N * ladder[0] + 1920 * (ladder[1] - ladder[0]) + 1920 * (ladder[2] - ladder[1])
    got = c["none"]
    assert got["level_pixels"] == [N, 0, 0] and (got["samples"] == ladder[0]).all()
    for f in FIELDS + ("rgba",):
        assert np.array_equal(_bits(got[f]), _bits(c["prefix"][ladder[0]][f])), f
    assert c["none_stats"]["primary_rays"] == N * ladder[0]


@pytest.mark.parametrize("top", (30, 32))
def test_rays_of_the_middle_threshold(hip, top):
    """primary_rays = width * height * P0 + the sum of padded length x (Pl - P(l-1)), strictly below what rendering every list from
    scratch costs, the sum of padded length x Pl."""
    c = _fused(hip, top)
    ladder, padded, lp = c["ladder"], c["host"]["padded"], c["fused"]["level_pixels"]
    assert padded[0] == N and [(n + 63) // 64 * 64 for n in lp[1:]] == padded[1:]
    want = N * ladder[0] + sum(p * (ladder[l] - ladder[l - 1]) for l, p in enumerate(padded) if l)
    scratch = sum(p * k for p, k in zip(padded, ladder))
    print("ladder", ladder, "primary rays kept", c["fused_stats"]["primary_rays"], "from scratch", scratch)
    assert c["fused_stats"]["primary_rays"] == want < scratch
    for k in ("secondary_rays", "shadow_rays", "shaded_hits"):
        assert 0 < c["fused_stats"][k] < c["all_stats"][k], k


def test_the_bits_do_not_depend_on_the_sample_group(hip):
    """The list passes of (8, 16, 32) hold 4 and 8 samples per slot over lists padded to 64 entries: they run with a sample group of 4
    and 8 (level 0 cannot: 3 800 slots are no multiple of 64 / G; the 3 samples per slot of (6, 14, 30) allow none either).  With
    rr_tuning::sample_group = 1 every pass runs ungrouped and returns the same frame; so does a prefix over a padded list."""
    c = _fused(hip, 32)
    cfg = _cfg("plain", samples=32)
    xy = _all_pixels_shuffled()[:128]
    with hip.DeviceScene(c["fs"], 0) as ds:
        grouped = ds.render_pixel_prefix(c["cam"], cfg, xy, samples_used=16, halves=True, rgba8=True)
        ds.set_tuning(sample_group=1)
        got = ds.render_adaptive_prefix(c["cam"], cfg, c["ladder"], c["threshold"], rgba8=True)
        st = ds.stats()
        single = ds.render_pixel_prefix(c["cam"], cfg, xy, samples_used=16, halves=True, rgba8=True)
    _same_frame(got, c["fused"], "sample_group 1", FIELDS + ("samples", "error", "rgba"))
    for k in COUNTERS:
        assert st[k] == c["fused_stats"][k], k
    _same(single, grouped, "a padded list at 16 of 32 samples", FIELDS + ("rgba",)); _same(single["parts"], grouped["parts"], "halves")
    _same(single, {f: c["prefix"][16][f][_index(xy)] for f in FIELDS + ("rgba",)}, "against the whole frame", FIELDS + ("rgba",))


def test_a_list_that_crosses_the_scans_carry(hip):
    """264 x 250 = 66 000 pixels, ladder (2, 4), threshold -1: 1 032 waves of entries, more than one step of the scan, all of them taken."""
    w, h = 264, 250
    fs = _scene("spheres_room")
    cam = camera_for(fs, w, h).c_struct()
    cfg = _cfg("plain", samples=4)
    with hip.DeviceScene(fs, 0) as ds:
        got = ds.render_adaptive_prefix(cam, cfg, (2, 4), -1.0, rgba8=True)
        st = ds.stats()
        want = ds.render_pixels(cam, cfg, None, rgba8=True)
    assert got["level_pixels"] == [w * h, w * h] and (got["samples"] == 4).all()
    assert st["primary_rays"] == w * h * 2 + ((w * h + 63) // 64 * 64) * 2
    for f in FIELDS + ("rgba",):
        assert np.array_equal(_bits(got[f]), _bits(want[f])), f


def test_fused_device_form_on_a_stream(hip):
    import torch
    from rustray_amd import renderer
    c = _fused(hip, 30)
    cam, cfg, want, ladder, thr = c["cam"], _cfg("plain", samples=30), c["fused"], c["ladder"], c["threshold"]
    L = hip.lib()
    lv = (C.c_uint16 * 3)(*ladder)
    with hip.DeviceScene(c["fs"], 0) as ds:
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            got = renderer.render_adaptive_prefix_torch(ds, cam, cfg, ladder, thr, rgba8=True)
        st.synchronize()
        rec = got["records"].cpu().numpy().view(np.uint32)
        assert got["level_pixels"] == want["level_pixels"] and rec.shape == (N, 8)
        assert np.array_equal(rec[:, 0:3], _bits(want["color"])) and np.array_equal(rec[:, 3], _bits(want["depth"]))
        assert np.array_equal(rec[:, 4:7], _bits(want["normal"])) and np.array_equal(rec[:, 7], want["object_id"])
        assert np.array_equal(got["samples"].cpu().numpy().astype(np.uint32), want["samples"])
        assert np.array_equal(_bits(got["error"].cpu().numpy()), _bits(want["error"])) and np.array_equal(got["rgba"].cpu().numpy(), want["rgba"])
        out = torch.full((N + 2, 8), SENTINEL, dtype=torch.int32, device="cuda")
        rgba = torch.full((N + 2,), SENTINEL, dtype=torch.int32, device="cuda")
        smp = torch.full((N + 2,), 0x5a5a, dtype=torch.int16, device="cuda")
        err = torch.full((N + 2,), SENTINEL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        level_pixels = (C.c_uint32 * 4)(77, 77, 77, 77)

        def call(o=None, r=None, s=None, e=None):
            return L.rr_render_adaptive_prefix_device(ds._h, C.byref(cam), C.byref(cfg), None, lv, 3, C.c_float(thr), C.c_void_p(o or out.data_ptr()),
                                                      C.c_void_p(r or rgba.data_ptr()), C.c_void_p(s or smp.data_ptr()), C.c_void_p(e or err.data_ptr()), level_pixels,
                                                      C.c_void_p(st.cuda_stream), None)
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
        only = torch.full((N + 2, 8), SENTINEL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert ds.render_adaptive_prefix_device(cam, cfg, ladder, thr, only.data_ptr(), stream_ptr=st.cuda_stream) == want["level_pixels"]
        st.synchronize()
        o = only.cpu().numpy().view(np.uint32)
        assert np.array_equal(o[:N], rec) and (o[N:] == SENTINEL).all()
        assert ds.stats()["primary_rays"] == c["fused_stats"]["primary_rays"]


def test_the_handle_afterwards(hip):
    c = _fused(hip, 30)
    fs, cam, ladder, thr = c["fs"], c["cam"], c["ladder"], c["threshold"]
    cfg, cfg6 = _cfg("plain", samples=30), _cfg("plain")
    keys = FIELDS + ("samples", "error", "rgba")

    def frames_equal(a, b, what):
        for k in ("rgba", "normal", "depth", "object_id"):
            assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)

    edited = _scene("spheres_room")
    for m in edited.materials:
        m.base_color, m.specular_color = tuple(m.specular_color), tuple(m.base_color)
        m.reflectivity = 0.25
    with hip.DeviceScene(fs, 0) as ds:
        first = ds.render(cam, cfg6, aux=True)
        got = ds.render_adaptive_prefix(cam, cfg, ladder, thr, rgba8=True)
        st = ds.stats()
        second = ds.render(cam, cfg6, aux=True)
        flag = C.c_int(1)
        with pytest.raises(hip.RustrayHipError) as ei:
            ds.render_adaptive_prefix(cam, cfg, ladder, thr, cancel=flag)
        assert ei.value.code == -6
        third = ds.render(cam, cfg6, aux=True)
        levels = ds.render_adaptive_levels(cam, cfg, ladder, thr, rgba8=True)        # the neighbouring call shares the lists and the scratch
        again = ds.render_adaptive_prefix(cam, cfg, ladder, thr, rgba8=True)
        ds.update_materials(edited.materials)
        after_edit = ds.render_adaptive_prefix(cam, cfg, ladder, thr, rgba8=True)
    with hip.DeviceScene(fs, 0) as fresh:
        want_levels = fresh.render_adaptive_levels(cam, cfg, ladder, thr, rgba8=True)
    with hip.DeviceScene(edited, 0) as fresh:
        want_edit = fresh.render_adaptive_prefix(cam, cfg, ladder, thr, rgba8=True)
    frames_equal(first, second, "after a fused call")
    frames_equal(first, third, "after a cancelled fused call")
    _same_frame(got, c["fused"], "between two frames", keys)
    _same_frame(again, c["fused"], "after rr_render_adaptive_levels", keys)
    _same_frame(levels, want_levels, "rr_render_adaptive_levels after the prefix call", keys)
    _same_frame(after_edit, want_edit, "after rr_scene_update_materials", keys)
    assert not np.array_equal(_bits(after_edit["color"]), _bits(got["color"]))
    for k in COUNTERS:
        assert st[k] == c["fused_stats"][k], k
