"""rr_render_pixels: Raytracing::render(x, y) before its clamp, as linear floats, for a list of pixels or for the whole frame.

One 50 x 38 frame (1 900 pixels: seven workgroups and a 108-slot tail) of three scenes under four configs, with the oracle's
sub-sample table.  The call is pinned from four sides: in float against the oracle's float64 means; bit for bit against rr_render of
the same handle, camera, config and table (depth, normal, id, and the frame's bytes through rgba8_out); word for word against
rr_shade_rays on the oracle's primary rays of that camera; and a list call against the whole-frame call, record by record."""
import ctypes as C

import numpy as np
import pytest

from rustray_amd.flat import make_config, rr_radiance
from tests.helpers import (BAND_EPS_ABS, BAND_EPS_REL, D6_CLAMP, U32, as_u8, camera_for, depth_check, item_transforms, load_scene, normal_check)
from tests.test_gpu_shade_rays import primaries, _scene

pytestmark = pytest.mark.gpu

W, H, SEED = 50, 38, 3
N = W * H
SCENES = ("rich", "spheres_room", "monkey")
CONFIGS = {
    "plain": dict(samples=3),
    "dof": dict(samples=3, focal_length=6.0, aperture_size=4.0),
    "dof_gamma16": dict(samples=16, focal_length=6.0, aperture_size=4.0, gamma_correction=True),   # the frame groups 16 samples of a pixel per packet
    "fog": dict(samples=3, fog_density=0.05),
}
CASES = [(s, c) for s in SCENES for c in CONFIGS]
ABOVE_ONE = {"plain": 642, "dof": 696, "dof_gamma16": 692, "fog": 156}   # spheres_room: channel means above 1 (CPU oracle)
COUNTERS = ("primary_rays", "secondary_rays", "shadow_rays", "shaded_hits")
FIELDS = ("color", "depth", "normal", "object_id")
SENTINEL = 0x5a5a5a5a
_cache = {}


def _cfg(config, **more):
    kw = dict(monte_carlo=True, seed=SEED, max_recursion=4)
    kw.update(CONFIGS[config]); kw.update(more)
    return make_config(**kw)


def _case(hip, oracle, name, config, need_ref=False):
    """One scene under one config, computed once on one handle: rr_render's frame, then the whole frame through rr_render_pixels,
    each with its counters; the oracle's frame with means and counters on request."""
    key = (name, config)
    if key not in _cache:
        fs = _scene(name)
        cam = camera_for(fs, W, H).c_struct()
        cfg = _cfg(config)
        table, _ = oracle.sample_table(cfg.samples)
        c = dict(fs=fs, cam=cam, cfg=cfg, table=table)
        with hip.DeviceScene(fs, 0) as ds:
            c["frame"] = ds.render(cam, cfg, sample_xy=table, aux=True); c["frame_stats"] = ds.stats()
            c["full"] = ds.render_pixels(cam, cfg, None, sample_xy=table, rgba8=True); c["full_stats"] = ds.stats()
        _cache[key] = c
    c = _cache[key]
    if need_ref and "ref" not in c:
        c["ref"] = oracle.render(c["fs"].c_struct(), c["cam"], c["cfg"], sample_xy=c["table"], want_means=True, want_counters=True, n_threads=8)
    return c


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b, what="", fields=FIELDS + ("rgba",)):
    for k in fields:
        assert a[k].shape == b[k].shape, (what, k, a[k].shape, b[k].shape)
        assert np.array_equal(_bits(a[k]), _bits(b[k])), f"{what}: {k} differs in {int((_bits(a[k]) != _bits(b[k])).sum())} words"


def _pick(res, idx):
    return {k: v[idx] for k, v in res.items()}


def _pack(x, y):
    return (np.asarray(x, np.uint32) | (np.asarray(y, np.uint32) << np.uint32(16))).astype(np.uint32)


def _index(xy):
    return (xy >> np.uint32(16)).astype(np.int64) * W + (xy & np.uint32(0xffff)).astype(np.int64)


def _all_pixels_shuffled(w=W, h=H, seed=11):
    ys, xs = np.divmod(np.arange(w * h), w)
    return _pack(xs, ys)[np.random.default_rng(seed).permutation(w * h)]


# ---- 1: against the oracle -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,config", CASES)
def test_against_the_oracles_float64_means(hip, oracle, name, config):
    """Every colour channel of every pixel inside the project's band around the oracle's float64 mean; nothing is skipped.
    Measured worst |color - m| / e on one MI355X (plain / dof / dof_gamma16 / fog): rich 0.1669 / 0.2751 / 0.2160 / 0.0535,
    spheres_room 0.0634 / 0.0792 / 0.0305 / 0.0444, monkey 0.0939 / 0.1127 / 0.0986 / 0.0399."""
    c = _case(hip, oracle, name, config, need_ref=True)
    ref, got, st = c["ref"], c["full"], c["full_stats"]
    S = c["cfg"].samples
    m = ref["mean_rgb"].reshape(N, 3)
    # nothing to skip: every mean is finite and no sample component is beyond the D6 clamp
    assert np.isfinite(m).all() and not (ref["max_abs_rgb"] > D6_CLAMP).any() and float(ref["max_abs_rgb"].max()) <= 7.8
    if name == "spheres_room":
        assert int((m > 1.0).sum()) == ABOVE_ONE[config]      # the float output must carry them unclamped
    assert np.array_equal(got["object_id"], ref["object_id"].reshape(N))
    e = BAND_EPS_REL * np.abs(m) + BAND_EPS_ABS + 4 * U32 * np.abs(m)   # the band of tests/helpers.py + the f32 rounding depth_check grants
    err = np.abs(got["color"].astype(np.float64) - m)
    worst = float((err / e).max())
    print(f"render_pixels {name} {config}: worst |color - m| / e = {worst:.4f}")
    assert (err <= e).all(), f"{name} {config}: {int((err > e).sum())} channels outside, worst |color - m| / e = {worst:.4f}"
    assert (got["color"][m > 1.0 + 1e-3] > 1.0).all()
    dc = depth_check(got["depth"], ref["depth"].reshape(N), ref["mean_depth"].reshape(N))
    nc = normal_check(got["normal"], ref["mean_normal"].reshape(N, 3))
    assert dc["n_depth_outside"] == 0 and nc["n_normal_outside"] == 0, (dc, nc, worst)
    assert np.array_equal(np.isnan(got["normal"]), np.isnan(ref["normal"].reshape(N, 3)))
    k = ref["counters"]
    assert st["primary_rays"] == k["rays_primary"] == N * S and st["secondary_rays"] == k["rays_secondary"] and st["shaded_hits"] == k["shaded_hits"], (st, k, worst)


# ---- 2: against rr_render --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,config", CASES)
def test_equals_the_frame(hip, oracle, name, config):
    c = _case(hip, oracle, name, config)
    got, frame = c["full"], c["frame"]
    assert np.array_equal(got["depth"], frame["depth"].reshape(N)), "depth"
    assert np.array_equal(got["normal"], frame["normal"].reshape(N, 3), equal_nan=True), "normal"
    assert np.array_equal(got["object_id"], frame["object_id"].reshape(N)), "object_id"
    want = frame["rgba"].reshape(N, 4)
    assert np.array_equal(got["rgba"], want), f"rgba8_out: {int((got['rgba'] != want).sum())} bytes differ from the frame's"
    if not c["cfg"].gamma_correction:
        v = np.fmin(got["color"].astype(np.float32), np.float32(1.0)) * np.float32(255.0)   # f32::min: NaN.min(1.0) = 1.0
        assert v.dtype == np.float32
        assert np.array_equal(as_u8(v).astype(np.uint8), want[:, :3])
    for k in COUNTERS:
        assert c["full_stats"][k] == c["frame_stats"][k], (k, c["full_stats"], c["frame_stats"])


# ---- 3: against rr_shade_rays ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,config", [("rich", "plain"), ("spheres_room", "dof"), ("monkey", "dof_gamma16")])
def test_equals_shade_rays_on_the_oracles_primaries(hip, oracle, name, config):
    """The frame's own camera against the caller's rays: the oracle's primary rays of this camera and config (the lens branch included),
    with stream id y * W + x, give the same records word for word."""
    c = _case(hip, oracle, name, config)
    o, d = primaries(oracle, c["cam"], c["cfg"], c["table"])
    with hip.DeviceScene(c["fs"], 0) as ds:
        rays = ds.shade_rays(o, d, c["cfg"], c["cfg"].samples, stream_ids=np.arange(N, dtype=np.uint32))
    _same(c["full"], rays, f"{name} {config}", fields=FIELDS)


# ---- 4: lists --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,config", [(s, c) for s in ("rich", "spheres_room") for c in ("plain", "dof_gamma16")])
def test_lists_equal_the_whole_frame_record_by_record(hip, oracle, name, config):
    """(With 16 samples a packet holds 4 pixels x 16 samples: 64 entries keep whole groups, 1, 63, 65 and 257 run without groups.)"""
    c = _case(hip, oracle, name, config)
    perm = _all_pixels_shuffled()
    ys, xs = np.mgrid[5:21, 7:32]
    rect = _pack(xs.reshape(-1), ys.reshape(-1))
    lists = {"permutation": perm, "rectangle": rect, "twice": np.repeat(perm[:300], 2), "twice, apart": np.concatenate([perm[:130], perm[:130]])}
    for k in (1, 63, 64, 65, 257):
        lists[f"prefix {k}"] = perm[:k]
    assert len(rect) == 25 * 16
    with hip.DeviceScene(c["fs"], 0) as ds:
        for what, xy in lists.items():
            got = ds.render_pixels(c["cam"], c["cfg"], xy, sample_xy=c["table"], rgba8=True)
            assert ds.stats()["primary_rays"] == len(xy) * c["cfg"].samples, what
            _same(got, _pick(c["full"], _index(xy)), f"{name} {config} {what}")
        # (x, y) pairs are the packed form
        pairs = np.stack([rect & 0xffff, rect >> 16], axis=1).astype(np.int64)
        _same(ds.render_pixels(c["cam"], c["cfg"], pairs, sample_xy=c["table"], rgba8=True), _pick(c["full"], _index(rect)), "pairs")


# ---- 5: batches ------------------------------------------------------------------------------------------------------------------
def test_batches_and_shade_chunks(hip, oracle):
    """152 x 120 x 16 = 291 840 primary rays under the two ray-memory budgets and the 65 536-ray shade chunks of
    tests/test_gpu_shade_rays.py: the whole frame and a shuffled list of all its pixels, in several batches, against one batch."""
    w, h, spp = 152, 120, 16
    fs = _scene("rich")
    cam = camera_for(fs, w, h).c_struct()
    cfg = _cfg("plain", samples=spp)
    table, _ = oracle.sample_table(spp)
    perm = _all_pixels_shuffled(w, h)
    slack = 2 * 256 * 5
    with hip.DeviceScene(fs, 0) as ds:
        whole = ds.render_pixels(cam, cfg, None, sample_xy=table, rgba8=True); wst = ds.stats()
        listed = ds.render_pixels(cam, cfg, perm, sample_xy=table, rgba8=True); lst = ds.stats()
        runs = []
        for b_max in (100000, 45000):
            ds.set_tuning(queue_budget_bytes=56 * (3 * b_max + slack), shade_chunk_rays=65536)
            a = ds.render_pixels(cam, cfg, None, sample_xy=table, rgba8=True); ast = ds.stats()
            b = ds.render_pixels(cam, cfg, perm, sample_xy=table, rgba8=True); bst = ds.stats()
            runs.append((a, ast, b, bst))
    idx = (perm >> np.uint32(16)).astype(np.int64) * w + (perm & np.uint32(0xffff)).astype(np.int64)
    assert wst["batches"] == 1 and lst["batches"] == 1 and wst["primary_rays"] == lst["primary_rays"] == 291840
    _same(listed, _pick(whole, idx), "the shuffled list in one batch")
    for a, ast, b, bst in runs:
        assert ast["batches"] > 1 and bst["batches"] > 1, (ast, bst)
        _same(a, whole, f"whole frame in {ast['batches']} batches")
        _same(b, listed, f"shuffled list in {bst['batches']} batches")
        for k in COUNTERS:
            assert ast[k] == bst[k] == wst[k] == lst[k], (k, ast, bst, wst, lst)


# ---- 6: the device form ----------------------------------------------------------------------------------------------------------
def _records(t):
    return t.cpu().numpy().view(np.uint32)


def test_device_form_equals_the_host_form(hip, oracle):
    import torch
    from rustray_amd import renderer
    c = _case(hip, oracle, "rich", "dof_gamma16")
    cam, cfg, table = c["cam"], c["cfg"], c["table"]
    perm = _all_pixels_shuffled()[:777]
    with hip.DeviceScene(c["fs"], 0) as ds:
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            txy = torch.from_numpy(perm.view(np.int32)).cuda()      # produced on this stream and not synchronised
            a = renderer.render_pixels_torch(ds, cam, cfg, txy, sample_xy=table, rgba8=True)
            b = renderer.render_pixels_torch(ds, cam, cfg, None, sample_xy=table, rgba8=True)
        st.synchronize()
        assert ds.stats()["primary_rays"] == N * cfg.samples
        for got, want, what in ((a, _pick(c["full"], _index(perm)), "a list on the device"), (b, c["full"], "the whole frame")):
            n = len(want["depth"])
            rec = _records(got["records"])
            assert rec.shape == (n, 8)
            assert np.array_equal(rec[:, 0:3], _bits(want["color"])) and np.array_equal(rec[:, 3], _bits(want["depth"])), what
            assert np.array_equal(rec[:, 4:7], _bits(want["normal"])) and np.array_equal(rec[:, 7], want["object_id"]), what
            assert np.array_equal(got["rgba"].cpu().numpy(), want["rgba"]), what
            # the named tensors are views of `records`
            for k, cols in (("color", slice(0, 3)), ("depth", 3), ("normal", slice(4, 7))):
                assert got[k].data_ptr() == got["records"][:, cols].data_ptr() and np.array_equal(_records(got[k].contiguous()), rec[:, cols]), (what, k)
            assert got["object_id"].dtype == torch.int32 and np.array_equal(got["object_id"].cpu().numpy().view(np.uint32), rec[:, 7])
        with pytest.raises((TypeError, ValueError)):
            renderer.render_pixels_torch(ds, cam, cfg, torch.from_numpy(perm.view(np.int32)), sample_xy=table)       # a host tensor
        with pytest.raises(TypeError):
            renderer.render_pixels_torch(ds, cam, cfg, txy.to(torch.int64), sample_xy=table)


def test_device_form_refusals_launch_nothing(hip, oracle):
    import torch
    c = _case(hip, oracle, "rich", "plain")
    cam, cfg, table = c["cam"], c["cfg"], c["table"]
    L = hip.lib()
    perm = _all_pixels_shuffled()[:257]
    tab = np.ascontiguousarray(table, np.uint16)
    with hip.DeviceScene(c["fs"], 0) as ds:
        txy = torch.from_numpy(perm.view(np.int32)).cuda()
        out = torch.full((257, 8), SENTINEL, dtype=torch.int32, device="cuda")
        rgba = torch.full((257,), SENTINEL, dtype=torch.int32, device="cuda")
        h_xy, h_out, h_rgba = perm.copy(), np.zeros((257, 8), np.float32), np.zeros((257, 4), np.uint8)   # pageable host memory

        def call(xy_p, n, out_p, rgba_p):
            return L.rr_render_pixels_device(ds._h, C.byref(cam), C.byref(cfg), tab.ctypes.data_as(C.c_void_p), C.c_void_p(xy_p) if xy_p else None, n,
                                             C.c_void_p(out_p) if out_p else None, C.c_void_p(rgba_p) if rgba_p else None, None, None)
        for args, arg in (((h_xy.ctypes.data, 257, out.data_ptr(), rgba.data_ptr()), b"pixel_xy_dev"),
                          ((txy.data_ptr(), 257, h_out.ctypes.data, rgba.data_ptr()), b"out_dev"),
                          ((txy.data_ptr(), 257, out.data_ptr(), h_rgba.ctypes.data), b"rgba8_out_dev")):
            assert call(*args) == -1 and arg in L.rr_last_error(), (arg, L.rr_last_error())
        assert call(txy.data_ptr(), 257, out.data_ptr() + 8, rgba.data_ptr()) == -1 and b"aligned" in L.rr_last_error()
        assert call(txy.data_ptr() + 2, 256, out.data_ptr(), rgba.data_ptr()) == -1 and b"aligned" in L.rr_last_error()
        assert call(txy.data_ptr(), 257, None, rgba.data_ptr()) == -1
        assert call(None, 257, out.data_ptr(), rgba.data_ptr()) == -1 and b"257" in L.rr_last_error()      # no list: the whole frame or nothing
        # entry 70 lies one column outside the frame (and so does a later one): refused by name, nothing written
        bad = perm.copy()
        bad[70] = np.uint32(W) | (np.uint32(5) << np.uint32(16))
        bad[200] = np.uint32(3) | (np.uint32(H) << np.uint32(16))
        tbad = torch.from_numpy(bad.view(np.int32)).cuda()
        assert call(tbad.data_ptr(), 257, out.data_ptr(), rgba.data_ptr()) == -1
        assert b"pixel_xy[70]" in L.rr_last_error(), L.rr_last_error()
        with pytest.raises(hip.RustrayHipError) as e:
            ds.render_pixels(cam, cfg, bad, sample_xy=table)        # the host form names the same entry
        assert e.value.code == -1 and "pixel_xy[70]" in str(e.value)
        # no pixels: RR_OK, no pointer is looked at
        assert call(None, 0, out.data_ptr(), None) == 0 and call(h_xy.ctypes.data, 0, h_out.ctypes.data, None) == 0
        torch.cuda.synchronize()
        assert (out.cpu().numpy().view(np.uint32) == SENTINEL).all() and (rgba.cpu().numpy().view(np.uint32) == SENTINEL).all()
        # and the handle answers afterwards
        assert call(txy.data_ptr(), 257, out.data_ptr(), rgba.data_ptr()) == 0
        torch.cuda.synchronize()
        want = _pick(c["full"], _index(perm))
        assert np.array_equal(_records(out)[:, 0:3], _bits(want["color"])) and np.array_equal(rgba.cpu().numpy().view(np.uint8).reshape(257, 4), want["rgba"])


# ---- 7: the handle afterwards ----------------------------------------------------------------------------------------------------
def test_the_handle_afterwards(hip, oracle):
    """A list call between two frames, and a whole-frame call between two frames: the second frame is the first (the cached region
    map is the frame's own), and both are a fresh handle's."""
    c = _case(hip, oracle, "rich", "plain")
    fs, cam, cfg, table = c["fs"], c["cam"], c["cfg"], c["table"]
    perm = _all_pixels_shuffled()
    rng = np.random.default_rng(7)
    o, d = primaries(oracle, cam, cfg, table[:1])
    po, pd = o[rng.integers(0, len(o), 256)], rng.normal(size=(256, 3)).astype(np.float32)

    def frame_and_queries(ds):
        f = ds.render(cam, cfg, sample_xy=table, aux=True)
        st = {k: ds.stats()[k] for k in COUNTERS}
        t = [_bits(x).tobytes() for x in ds.trace_rays(po, pd, 1)]
        r = ds.shade_rays(o[:300], d[:300], cfg, 3)
        return f, st, t, [_bits(r[k]).tobytes() for k in FIELDS]

    def same_frames(a, b, what):
        for k in ("rgba", "normal", "depth", "object_id"):
            assert np.array_equal(a[0][k], b[0][k], equal_nan=True), (what, k)
        assert a[1:] == b[1:], what

    with hip.DeviceScene(fs, 0) as ds:
        first = frame_and_queries(ds)
        got65 = ds.render_pixels(cam, cfg, perm[:65], sample_xy=table, rgba8=True)
        second = frame_and_queries(ds)
        whole = ds.render_pixels(cam, cfg, None, sample_xy=table, rgba8=True)
        third = frame_and_queries(ds)
        # another frame shape right after a list call of this one
        ds.render_pixels(cam, cfg, perm[:65], sample_xy=table)
        cam2, cfg2 = camera_for(fs, 64, 48).c_struct(), _cfg("plain", samples=4)
        small_after = ds.render(cam2, cfg2, aux=True)
    with hip.DeviceScene(fs, 0) as fresh:
        want = frame_and_queries(fresh)
    with hip.DeviceScene(fs, 0) as fresh:
        small_want = fresh.render(cam2, cfg2, aux=True)
    same_frames(first, second, "after a list of 65 pixels")
    same_frames(first, third, "after a whole-frame call")
    same_frames(first, want, "a fresh handle")
    _same(got65, _pick(c["full"], _index(perm[:65])), "65 pixels between two frames")
    _same(whole, c["full"], "the whole frame between two frames")
    for k in ("rgba", "normal", "depth", "object_id"):
        assert np.array_equal(small_after[k], small_want[k], equal_nan=True), k


def test_an_edit_waits_for_the_call_in_flight(hip, oracle):
    import torch
    from tests.helpers import with_transforms
    fs = load_scene("spheres_room")
    cam, cfg = camera_for(fs, W, H).c_struct(), _cfg("plain")
    table, _ = oracle.sample_table(cfg.samples)
    t, ti = item_transforms(fs, dx=0.4)
    perm = _all_pixels_shuffled()
    with hip.DeviceScene(fs, 0) as ref:
        unedited = ref.render_pixels(cam, cfg, perm, sample_xy=table, rgba8=True)
    with hip.DeviceScene(with_transforms(load_scene("spheres_room"), t, ti), 0) as ref:
        edited = ref.render_pixels(cam, cfg, perm, sample_xy=table, rgba8=True)
    assert not np.array_equal(_bits(unedited["color"]), _bits(edited["color"]))
    with hip.DeviceScene(fs, 0) as ds:
        ds.render_pixels(cam, cfg, perm[:64], sample_xy=table)                     # first use: the handle's buffers exist
        txy = torch.from_numpy(perm.view(np.int32)).cuda()
        out = torch.full((N, 8), SENTINEL, dtype=torch.int32, device="cuda")
        rgba = torch.full((N,), SENTINEL, dtype=torch.int32, device="cuda")
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        ds.render_pixels_device(cam, cfg, txy.data_ptr(), N, out.data_ptr(), rgba.data_ptr(), st.cuda_stream, sample_xy=table)
        ds.update_transforms(t, ti)                                              # at once: the edit must wait for what the call still reads
        torch.cuda.synchronize()
        rec = _records(out)
        assert np.array_equal(rec[:, 0:3], _bits(unedited["color"])) and np.array_equal(rec[:, 3], _bits(unedited["depth"]))
        assert np.array_equal(rgba.cpu().numpy().view(np.uint8).reshape(N, 4), unedited["rgba"])
        _same(ds.render_pixels(cam, cfg, perm, sample_xy=table, rgba8=True), edited, "the same call after the edit")


# ---- 8: arguments ----------------------------------------------------------------------------------------------------------------
def test_argument_errors(hip, oracle):
    c = _case(hip, oracle, "spheres_room", "plain")
    cam, cfg, table = c["cam"], c["cfg"], c["table"]
    L = hip.lib()
    perm = _all_pixels_shuffled()[:130]
    big_table = np.zeros((32767, 2), np.uint16)
    with hip.DeviceScene(c["fs"], 0) as ds:
        out = (rr_radiance * N)()
        C.memset(out, 0x5a, C.sizeof(out))
        tab_p, xy_p = np.ascontiguousarray(table, np.uint16).ctypes.data_as(C.c_void_p), perm.ctypes.data_as(C.c_void_p)

        def call(cfg_, table_p, xy, n, o=out, cancel=None):
            return L.rr_render_pixels(ds._h, C.byref(cam), C.byref(cfg_), table_p, xy, n, o, None, cancel)
        # without a list the call is the whole frame
        for n in (N - 1, N + 1, 1):
            assert call(cfg, tab_p, None, n) == -1 and b"without a list" in L.rr_last_error()
        # the frame's own limits: samples 0, samples beyond the table limit (with and without the caller's table), max_recursion
        assert call(_cfg("plain", samples=0), tab_p, xy_p, 130) == -1 and b"samples" in L.rr_last_error()
        assert call(_cfg("plain", samples=32767), big_table.ctypes.data_as(C.c_void_p), xy_p, 130) == -2 and b"samples" in L.rr_last_error()
        assert call(_cfg("plain", samples=16383), None, xy_p, 130) == -2 and b"samples" in L.rr_last_error()
        assert call(_cfg("plain", max_recursion=31), tab_p, xy_p, 130) == -2 and b"max_recursion" in L.rr_last_error()
        assert call(cfg, tab_p, xy_p, 130, o=None) == -1
        assert call(cfg, tab_p, xy_p, (1 << 30) + 1) == -2
        assert call(cfg, tab_p, None, 0) == 0 and call(cfg, tab_p, xy_p, 0) == 0
        # a cancel flag already set
        flag = C.c_int(1)
        assert call(cfg, tab_p, xy_p, 130, cancel=C.byref(flag)) == -6
        with pytest.raises(hip.RustrayHipError) as e:
            ds.render_pixels(cam, cfg, None, sample_xy=table, cancel=flag)
        assert e.value.code == -6
        assert bytes(out) == b"\x5a" * C.sizeof(out)
        _same(ds.render_pixels(cam, cfg, perm, sample_xy=table, rgba8=True, cancel=C.c_int(0)), _pick(c["full"], _index(perm)), "after the cancelled calls")
        # from on_pass of the same scene
        seen = []

        def on_pass(frame, done, total):
            with pytest.raises(hip.RustrayHipError) as e2:
                ds.render_pixels(cam, cfg, perm[:3], sample_xy=table)
            seen.append(e2.value.code)
            seen.append(L.rr_render_pixels_device(ds._h, C.byref(cam), C.byref(cfg), tab_p, None, N, out, None, None, None))
            return False
        ds.render_progressive(cam, _cfg("plain", samples=4), on_pass, min_passes=2)
        assert seen and all(code == -1 for code in seen)
        _same(ds.render_pixels(cam, cfg, None, sample_xy=table, rgba8=True), c["full"], "after the progressive frame")
        # gamma_correction reaches the bytes and nothing else
        g = ds.render_pixels(cam, _cfg("plain", gamma_correction=True), None, sample_xy=table, rgba8=True)
        _same(g, c["full"], "gamma_correction and the floats", fields=FIELDS)
        assert not np.array_equal(g["rgba"], c["full"]["rgba"])
