"""rr_shade_rays: Raytracing::get_color_depth_normal_id(scene, ray, 1) for caller-supplied rays, as linear floats per result.

The rays of cases 1 to 6 are the oracle's own primaries (rro_primary_ray, un-normalised directions) of a 50 x 38 frame with 3
samples per pixel in row-major pixel order: 5700 rays, a partial last packet and a sample count that does not divide 64.  Result
y * w + x is then that frame's pixel, which pins the call twice: per result in float against the oracle's float64 means (no channel,
pixel or result is skipped: the means of the three base cases are finite and inside the D6 clamp), and bit for bit against rr_render
of the same camera, config and sub-sample table (the same f32 operations, and integer accumulation does not depend on order)."""
import copy
import ctypes as C

import numpy as np
import pytest

from rustray_amd.flat import make_config, rr_radiance
from tests.helpers import (BAND_EPS_ABS, BAND_EPS_REL, D6_CLAMP, U32, as_u8, camera_for, depth_check, load_scene, normal_check)

pytestmark = pytest.mark.gpu

W, H, S, SEED = 50, 38, 3, 3
BASE = ("rich", "spheres_room", "monkey")
COUNTERS = ("primary_rays", "secondary_rays", "shadow_rays", "shaded_hits")
_cache = {}


def _scene(name):
    if name == "rich":
        from tools.fuzz_parity import rich_scene   # 20 items, 4 lights, every texture map: the packet form of the top level
        return rich_scene(9119)
    return load_scene(name)                        # spheres_room: 14 items, the per-ray walk; monkey: one mesh, mostly misses


def _cfg(samples=S):
    return make_config(samples=samples, monte_carlo=True, seed=SEED, max_recursion=4)


def primaries(oracle, cam, cfg, table):
    """The oracle's primary rays of every pixel (row-major) and every entry of `table`: (w * h * len(table), 3) origins and
    un-normalised directions; ray (y * w + x) * len(table) + k is sample k of pixel (x, y)."""
    fn = oracle.lib().rro_primary_ray
    fn.restype = None
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint16, C.c_uint16, C.c_void_p, C.c_void_p]
    n = cam.width * cam.height * len(table)
    o = np.zeros((n, 3), np.float32); d = np.zeros((n, 3), np.float32)
    cp, gp, po, pd = C.addressof(cam), C.addressof(cfg), o.ctypes.data, d.ctypes.data
    tab = [(int(a), int(b)) for a, b in table]
    i = 0
    for y in range(cam.height):
        for x in range(cam.width):
            for xi, yi in tab:
                fn(cp, gp, x, y, xi, yi, po + 12 * i, pd + 12 * i)
                i += 1
    return o, d


def _case(hip, oracle, name, samples=S, w=W, h=H, need_ref=True):
    """One scene at one sample count, computed once: the rays, the oracle's frame with its means and counters, rr_render's frame
    and rr_shade_rays' answer with their counters (one handle, frame first)."""
    key = (name, samples, w, h)
    if key not in _cache:
        fs = _scene(name)
        cam = camera_for(fs, w, h).c_struct()
        cfg = _cfg(samples)
        table, _ = oracle.sample_table(samples)
        o, d = primaries(oracle, cam, cfg, table)
        c = dict(fs=fs, cam=cam, cfg=cfg, table=table, o=o, d=d)
        with hip.DeviceScene(fs, 0) as ds:
            c["frame"] = ds.render(cam, cfg, sample_xy=table, aux=True); c["frame_stats"] = ds.stats()
            c["got"] = ds.shade_rays(o, d, cfg, samples); c["got_stats"] = ds.stats()
        _cache[key] = c
    c = _cache[key]
    if need_ref and "ref" not in c:
        c["ref"] = oracle.render(c["fs"].c_struct(), c["cam"], c["cfg"], sample_xy=c["table"], want_means=True, want_counters=True, n_threads=8)
    return c


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same_radiance(a, b, what=""):
    for k in ("color", "depth", "normal", "object_id"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), f"{what}: {k} differs in {int((_bits(a[k]) != _bits(b[k])).sum())} words"


def _equals_frame(got, frame, what=""):
    """depth, normal (NaN where the frame has NaN) and object_id array-equal; as_u8(min(color, 1) * 255) in float32 = the frame's bytes."""
    n = got["depth"].shape[0]
    assert np.array_equal(got["depth"], frame["depth"].reshape(n)), f"{what}: depth"
    assert np.array_equal(got["normal"], frame["normal"].reshape(n, 3), equal_nan=True), f"{what}: normal"
    assert np.array_equal(got["object_id"], frame["object_id"].reshape(n)), f"{what}: object_id"
    c = np.fmin(got["color"].astype(np.float32), np.float32(1.0)) * np.float32(255.0)   # f32::min: NaN.min(1.0) = 1.0
    assert c.dtype == np.float32
    bytes_ = as_u8(c).astype(np.uint8)
    want = frame["rgba"].reshape(n, 4)
    assert np.array_equal(bytes_, want[:, :3]), f"{what}: {int((bytes_ != want[:, :3]).sum())} colour bytes differ"


# ---- 1: against the oracle -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BASE)
def test_against_the_oracles_float64_means(hip, oracle, name):
    """Measured worst |color - m| / e per case (e = the bound below): rich 0.1669, spheres_room 0.0634, monkey 0.0939 (one MI355X)."""
    c = _case(hip, oracle, name)
    ref, got, st = c["ref"], c["got"], c["got_stats"]
    n = W * H
    m = ref["mean_rgb"].reshape(n, 3)
    # nothing to skip: every mean is finite and no sample component is beyond the D6 clamp
    assert np.isfinite(m).all() and not (ref["max_abs_rgb"] > D6_CLAMP).any()
    if name == "spheres_room":
        assert int((m > 1.0).sum()) == 642      # the float output must carry them unclamped
    assert np.array_equal(got["object_id"], ref["object_id"].reshape(n))
    e = BAND_EPS_REL * np.abs(m) + BAND_EPS_ABS + 4 * U32 * np.abs(m)   # the band of tests/helpers.py + the f32 rounding depth_check grants
    err = np.abs(got["color"].astype(np.float64) - m)
    worst = float((err / e).max())
    print(f"shade_rays {name}: worst |color - m| / e = {worst:.4f}")
    assert (err <= e).all(), f"{name}: {int((err > e).sum())} channels outside, worst |color - m| / e = {worst:.4f}"
    if name == "spheres_room":
        assert (got["color"][m > 1.0 + 1e-3] > 1.0).all()
    dc = depth_check(got["depth"], ref["depth"].reshape(n), ref["mean_depth"].reshape(n))
    nc = normal_check(got["normal"], ref["mean_normal"].reshape(n, 3))
    assert dc["n_depth_outside"] == 0 and nc["n_normal_outside"] == 0, (dc, nc, worst)
    assert np.array_equal(np.isnan(got["normal"]), np.isnan(ref["normal"].reshape(n, 3)))
    k = ref["counters"]
    assert st["primary_rays"] == k["rays_primary"] == n * S and st["secondary_rays"] == k["rays_secondary"] and st["shaded_hits"] == k["shaded_hits"], (st, k, worst)
    assert 0 < st["shadow_rays"] <= k["rays_shadow"], (st, k, worst)


# ---- 2: against rr_render --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,samples", [(n, S) for n in BASE] + [("rich", 16)])
def test_equals_the_frame_of_the_same_rays(hip, oracle, name, samples):
    """(rich at 16 samples: the frame groups 16 samples of a pixel per packet, the query does not.)"""
    c = _case(hip, oracle, name, samples, need_ref=False)
    _equals_frame(c["got"], c["frame"], f"{name} x{samples}")
    for k in COUNTERS:
        assert c["got_stats"][k] == c["frame_stats"][k], (k, c["got_stats"], c["frame_stats"])


# ---- 3: batching and tuning ------------------------------------------------------------------------------------------------------
def test_batches_and_shade_chunks(hip, oracle):
    """152 x 120 x 16 = 291 840 rays under two ray-memory budgets: 3 batches of 97 280 rays, each level 1 shaded in two chunks of at
    most 65 536 rays; and 7 batches of 41 692 rays, which cut results apart (41 692 is no multiple of 16)."""
    w, h, spp = 152, 120, 16
    fs = _scene("rich")
    cam = camera_for(fs, w, h).c_struct()
    cfg = _cfg(spp)
    table, _ = oracle.sample_table(spp)
    o, d = primaries(oracle, cam, cfg, table)
    assert len(o) == 291840 and -(-291840 // 3) == 97280 and -(-291840 // 7) == 41692 and 41692 % spp != 0
    slack = 2 * 256 * 5                                           # plan_ray_batches: 2 * RR_BLOCK * (max_recursion + 1)
    with hip.DeviceScene(fs, 0) as ds:
        frame = ds.render(cam, cfg, sample_xy=table, aux=True); fst = ds.stats()
        whole = ds.shade_rays(o, d, cfg, spp); wst = ds.stats()
        runs = []
        for b_max in (100000, 45000):
            ds.set_tuning(queue_budget_bytes=56 * (3 * b_max + slack), shade_chunk_rays=65536)
            runs.append((ds.shade_rays(o, d, cfg, spp), ds.stats()))
    assert wst["batches"] == 1 and [st["batches"] for _, st in runs] == [3, 7]
    for got, st in runs:
        _equals_frame(got, frame, f"{st['batches']} batches")
        _same_radiance(got, whole, f"{st['batches']} batches vs one batch")
        for k in COUNTERS:
            assert st[k] == fst[k] == wst[k], (k, st, fst, wst)
    assert fst["primary_rays"] == 291840 and fst["secondary_rays"] > 0 and fst["shadow_rays"] > 0


# ---- 4: stream ids ---------------------------------------------------------------------------------------------------------------
def test_stream_ids(hip, oracle):
    c = _case(hip, oracle, "rich", need_ref=False)
    n = W * H
    o3, d3 = c["o"].reshape(n, S, 3), c["d"].reshape(n, S, 3)
    ids = np.arange(n, dtype=np.uint32)
    x0, y0, ww, wh = 17, 11, 16, 8
    win = np.array([y * W + x for y in range(y0, y0 + wh) for x in range(x0, x0 + ww)], np.uint32)
    with hip.DeviceScene(c["fs"], 0) as ds:
        rev = ds.shade_rays(o3[::-1], d3[::-1], c["cfg"], S, stream_ids=ids[::-1])
        part = ds.shade_rays(o3[win], d3[win], c["cfg"], S, stream_ids=win)
        shifted = ds.shade_rays(c["o"], c["d"], c["cfg"], S, stream_ids=ids + np.uint32(0x80000000))   # other pixels: other draws
    _same_radiance({k: v[::-1] for k, v in rev.items()}, c["got"], "reversed results with reversed ids")
    _same_radiance(part, {k: v[win] for k, v in c["got"].items()}, "a 16 x 8 window with its frame ids")
    frame_win = {k: c["frame"][k][y0:y0 + wh, x0:x0 + ww] for k in ("rgba", "normal", "depth", "object_id")}
    _equals_frame(part, frame_win, "window vs frame")
    assert not np.array_equal(_bits(shifted["color"]), _bits(c["got"]["color"]))   # the ids reach the generator (Monte Carlo materials), all 32 bits of them
    assert np.array_equal(shifted["object_id"], c["got"]["object_id"])


# ---- 5: directions are used up to length -----------------------------------------------------------------------------------------
def test_direction_length_does_not_matter(hip, oracle):
    c = _case(hip, oracle, "spheres_room", need_ref=False)
    n = W * H
    o = np.concatenate([c["o"]] * 3)
    d = np.concatenate([c["d"], c["d"] * np.float32(4.0), c["d"] * np.float32(0.25)])
    ids = np.tile(np.arange(n, dtype=np.uint32), 3)
    with hip.DeviceScene(c["fs"], 0) as ds:
        got = ds.shade_rays(o, d, c["cfg"], S, stream_ids=ids)
    for b in range(3):
        _same_radiance({k: v[b * n:(b + 1) * n] for k, v in got.items()}, c["got"], f"block {b}")


# ---- 6: the handle afterwards ----------------------------------------------------------------------------------------------------
def test_the_handle_afterwards(hip, oracle):
    c = _case(hip, oracle, "rich", need_ref=False)
    fs, cam, cfg, table = c["fs"], c["cam"], c["cfg"], c["table"]
    rng = np.random.default_rng(7)
    po = c["o"][rng.integers(0, len(c["o"]), 256)]
    pd = rng.normal(size=(256, 3)).astype(np.float32)

    def queries(ds):
        f = ds.render(cam, cfg, sample_xy=table, aux=True)
        st = {k: ds.stats()[k] for k in COUNTERS}
        p = ds.pick(cam, W // 2, H // 2)
        t = ds.trace_rays(po, pd, 1)
        return f, st, (p.hit, p.object_id, p.item_index, p.distance), [_bits(x).tobytes() for x in t]

    with hip.DeviceScene(fs, 0) as ds:
        before = queries(ds)
        got = ds.shade_rays(c["o"], c["d"], cfg, S)
        after = queries(ds)
        # another frame shape and sample count after the query: the region map and the sub-sample table are the frame's own again
        cam2, cfg2 = camera_for(fs, 64, 48).c_struct(), _cfg(4)
        small_after = ds.render(cam2, cfg2, aux=True)
        lights = [copy.copy(l) for l in fs.lights]
        k = next(i for i, l in enumerate(lights) if l.enabled)
        lights[k].enabled = False
        ds.update_lights(lights)
        edited = ds.shade_rays(c["o"], c["d"], cfg, S)
    _same_radiance(got, c["got"], "the query between two frames")
    for k in ("rgba", "normal", "depth", "object_id"):
        assert np.array_equal(before[0][k], after[0][k], equal_nan=True), k
    assert before[1:] == after[1:]
    fs2 = _scene("rich")          # (built anew: a flat scene that has been handed to the library holds ctypes arrays and cannot be copied)
    fs2.lights = lights
    with hip.DeviceScene(fs2, 0) as fresh:
        want = fresh.shade_rays(c["o"], c["d"], cfg, S)
        small_fresh = fresh.render(cam2, cfg2, aux=True)
    _same_radiance(edited, want, "after rr_scene_update_lights vs a fresh handle")
    assert not np.array_equal(_bits(edited["color"]), _bits(got["color"]))
    with hip.DeviceScene(fs, 0) as fresh:
        small_want = fresh.render(cam2, cfg2, aux=True)
    for k in ("rgba", "normal", "depth", "object_id"):
        assert np.array_equal(small_after[k], small_want[k], equal_nan=True), k
    assert not np.array_equal(small_fresh["rgba"], small_want["rgba"])


# ---- 7: edges --------------------------------------------------------------------------------------------------------------------
def test_edges_and_argument_errors(hip, oracle):
    c = _case(hip, oracle, "spheres_room", need_ref=False)
    cfg, o, d = c["cfg"], c["o"], c["d"]
    L = hip.lib()
    with hip.DeviceScene(_scene("monkey"), 0) as ds:
        # one result of one ray that misses
        r = ds.shade_rays(np.array([[0, 1e6, 0]], np.float32), np.array([[0, 1, 0]], np.float32), cfg, 1)
        assert (r["color"] == 0).all() and r["depth"][0] == 0 and np.isnan(r["normal"]).all() and r["object_id"][0] == 0
        st = ds.stats()
        assert st["primary_rays"] == 1 and st["shaded_hits"] == 0 and st["batches"] == 1
    with hip.DeviceScene(c["fs"], 0) as ds:
        # n_results == 0 leaves `out` untouched, and not even NULL arrays are looked at
        out = (rr_radiance * 2)()
        C.memset(out, 0x5a, C.sizeof(out))
        assert L.rr_shade_rays(ds._h, C.byref(cfg), None, None, 0, 3, None, out, None) == 0
        assert bytes(out) == b"\x5a" * 64
        empty = ds.shade_rays(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), cfg, 3)
        assert len(empty["depth"]) == 0 and empty["color"].shape == (0, 3)
        op, dp = o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p)
        for rpr, code in ((0, -1), (32767, -2)):
            assert L.rr_shade_rays(ds._h, C.byref(cfg), op, dp, 2, rpr, None, out, None) == code
            assert b"rays_per_result" in L.rr_last_error()
        assert L.rr_shade_rays(ds._h, C.byref(cfg), op, dp, 0x7fffff01, 1, None, out, None) == -2
        deep = make_config(samples=1, max_recursion=31)
        assert L.rr_shade_rays(ds._h, C.byref(deep), op, dp, 2, 1, None, out, None) == -2 and b"max_recursion" in L.rr_last_error()
        for args in ((None, dp, out), (op, None, out), (op, dp, None)):
            assert L.rr_shade_rays(ds._h, C.byref(cfg), args[0], args[1], 2, 1, None, args[2], None) == -1
        # the ignored config fields are ignored
        other = make_config(samples=77, monte_carlo=True, seed=SEED, max_recursion=4, focal_length=3.0, aperture_size=2.0, gamma_correction=True)
        _same_radiance(ds.shade_rays(o, d, other, S), c["got"], "samples, focal_length, aperture_size, gamma_correction")
        # a cancel flag already set, and the call after it
        flag = C.c_int(1)
        with pytest.raises(hip.RustrayHipError) as e:
            ds.shade_rays(o, d, cfg, S, cancel=flag)
        assert e.value.code == -6
        _same_radiance(ds.shade_rays(o, d, cfg, S, cancel=C.c_int(0)), c["got"], "after a cancelled call")
        # from on_pass of the same scene
        seen = []

        def on_pass(frame, done, total):
            with pytest.raises(hip.RustrayHipError) as e2:
                ds.shade_rays(o[:3], d[:3], cfg, 3)
            seen.append(e2.value.code)
            return False
        ds.render_progressive(c["cam"], _cfg(4), on_pass, min_passes=2)
        assert seen and all(code == -1 for code in seen)
        _same_radiance(ds.shade_rays(o, d, cfg, S), c["got"], "after the progressive frame")


def test_non_finite_rays_are_answered(hip, oracle):
    """Rays with NaN and infinite components among ordinary ones: the call returns, and the ordinary results are unchanged."""
    c = _case(hip, oracle, "spheres_room", need_ref=False)
    n = 64
    o, d = c["o"][:n * S].copy(), c["d"][:n * S].copy()
    o[0 * S] = np.nan; d[1 * S + 1, 0] = np.inf; o[2 * S + 2, 1] = -np.inf; d[3 * S] = 0.0
    with hip.DeviceScene(c["fs"], 0) as ds:
        got = ds.shade_rays(o, d, c["cfg"], S)
    keep = np.arange(4, n)
    _same_radiance({k: v[keep] for k, v in got.items()}, {k: v[keep] for k, v in c["got"].items()}, "results without a non-finite ray")


def test_host_failure_returns_an_error(hip, oracle):
    """The fault point next to the call's host staging (as tests/test_gpu_guard.py): a status code comes back and the handle answers as before."""
    c = _case(hip, oracle, "spheres_room", need_ref=False)
    L = hip.lib()
    L.rr_test_fault.argtypes = [C.c_char_p, C.c_int, C.c_int]
    with hip.DeviceScene(c["fs"], 0) as ds:
        try:
            for kind, code in ((1, -5), (2, -4)):
                assert L.rr_test_fault(b"shade_rays.host", kind, 0) == 0
                with pytest.raises(hip.RustrayHipError) as e:
                    ds.shade_rays(c["o"], c["d"], c["cfg"], S)
                assert e.value.code == code and "rr_shade_rays" in str(e.value), str(e.value)
        finally:
            assert L.rr_test_fault(b"", 0, 0) == 0
        _same_radiance(ds.shade_rays(c["o"], c["d"], c["cfg"], S), c["got"], "after the failures")
