"""rr_albedo_pixels on the GPU: the frame's albedo per pixel, bit for bit mean_albedo (rustray_amd/albedo.py) of the base colours
rr_surface_rays gives for the frame's own primary rays -- the oracle's primaries of the same camera, config and sub-sample table,
normalised in binary32 (tests/test_gpu_surface_rays.py shows these are the frame's rays bit for bit).  No channel and no pixel is skipped.

Frames of 50x38 = 1900 pixels (a partial last packet): rich_scene(9119) (20 items, the packet top level, every texture map), spheres_room
(14 items, the per-ray walk), the checkered floor of tests/test_gpu_denoise_albedo.py; 3 samples (G = 1: the count does not divide 64),
4 samples (G = 4: the merged adds), 8 samples with depth of field, and once a caller's table."""
import ctypes as C

import numpy as np
import pytest
import torch

from rustray_amd import renderer
from rustray_amd.albedo import mean_albedo
from rustray_amd.flat import make_config
from tests.helpers import assert_frames_identical, camera_for, load_scene
from tests.test_gpu_denoise_albedo import _checkered_floor
from tests.test_gpu_shade_rays import primaries
from tests.test_gpu_surface_rays import _f32_normalised

pytestmark = pytest.mark.gpu

W, H = 50, 38
N = W * H
F = np.float32
SENTINEL = 0x5a
SCENES = ("rich", "spheres_room", "floor")
_scenes = {}
_cache = {}


def _scene(name):
    if name not in _scenes:
        if name == "rich":
            from tools.fuzz_parity import rich_scene
            _scenes[name] = rich_scene(9119)
        elif name == "floor":
            _scenes[name] = _checkered_floor()
        else:
            _scenes[name] = load_scene(name)
    return _scenes[name]


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _cfg(samples, dof=False):
    # seed, monte_carlo, max_recursion and the fog are set to what the call must ignore
    return make_config(samples=samples, monte_carlo=True, seed=77, max_recursion=4, fog_density=0.02,
                       focal_length=4.0 if dof else 1.0, aperture_size=2.5 if dof else 1.0)


def _table(oracle, samples, own):
    table, _ = oracle.sample_table(samples)
    table = np.ascontiguousarray(table, np.uint16).reshape(samples, 2)
    if own:    # a caller's table: every cell of the built-in one mirrored, in reverse order
        cell = int(table.max()) + 1
        table = np.ascontiguousarray((cell - 1 - table)[::-1])
    return table


def _case(hip, oracle, name, samples, dof=False, own=False):
    """One scene at one config, computed once and left unchanged: the expected albedo and the whole-frame answer of the host form."""
    key = (name, samples, dof, own)
    if key not in _cache:
        fs = _scene(name)
        cam = camera_for(fs, W, H).c_struct()
        cfg = _cfg(samples, dof)
        table = _table(oracle, samples, own)
        o, d = primaries(oracle, cam, cfg, table)
        assert len(o) == N * samples
        with hip.DeviceScene(fs, 0) as ds:
            surf = ds.surface_rays(o, _f32_normalised(d), 1)
            got = ds.albedo_pixels(cam, cfg, sample_xy=table if own else None)
            stats = ds.stats()
        base = np.ascontiguousarray(surf["base_color"][:, :3]).reshape(N, samples, 3)
        hit = (surf["hit"] == 1).reshape(N, samples)
        assert not base[~hit].any()                                  # a miss contributes 0
        want = mean_albedo(base, samples)
        for a in (want, got):
            a.setflags(write=False)
        _cache[key] = dict(fs=fs, cam=cam, cfg=cfg, table=table, want=want, got=got, hit=hit, stats=stats, sample_xy=table if own else None)
    return _cache[key]


CASES = [(name, s, dof, False) for name in SCENES for s, dof in ((3, False), (4, False), (8, True))] + [("rich", 4, False, True)]


@pytest.mark.parametrize("name,samples,dof,own", CASES)
def test_bit_for_bit_mean_of_the_surface_records_of_the_frames_rays(hip, oracle, name, samples, dof, own):
    c = _case(hip, oracle, name, samples, dof, own)
    got, want = c["got"], c["want"]
    assert got.shape == (N, 3) and got.dtype == np.float32
    assert np.isfinite(want).all()
    mixed = c["hit"].any(axis=1) & ~c["hit"].all(axis=1)
    assert c["hit"].any() and (name != "rich" or ((~c["hit"]).any() and mixed.any()))        # the textured frame has a background and silhouettes
    differ = _bits(got) != _bits(want)
    assert not differ.any(), (f"{int(differ.any(axis=1).sum())} of {N} pixels differ, the first at {int(np.argmax(differ.any(axis=1)))}: "
                              f"got {got[differ.any(axis=1)][:1]}, want {want[differ.any(axis=1)][:1]}, "
                              f"largest |difference| {float(np.abs(got.astype(np.float64) - want).max())}")
    assert len(np.unique(want[c["hit"].any(axis=1)], axis=0)) > 1
    st = c["stats"]
    assert st["primary_rays"] == N * samples and st["secondary_rays"] == 0 and st["shadow_rays"] == 0 and st["shaded_hits"] == 0


def test_the_mean_differs_from_the_centre_at_edges_only_by_mixing(hip, oracle):
    """S = 1 and sample_xy = [(0, 0)] on a camera without depth of field: the one ray passes through the pixel's centre, so the call is
    rr_surface_pixels' albedo but for the rounding of one term to 24 fractional bits: at most 2^-25 for a value below 1 (the sum is an
    integer below 2^24 and converts exactly); for a value in [1, 2) the sum has 25 bits and its conversion to binary32 adds at most
    another 2^-25."""
    for name in ("rich", "floor"):
        fs = _scene(name)
        cam = camera_for(fs, W, H).c_struct()
        with hip.DeviceScene(fs, 0) as ds:
            got = ds.albedo_pixels(cam, _cfg(1), sample_xy=np.zeros((1, 2), np.uint16))
            centre = ds.surface_pixels(cam, records=False, albedo=True)
        assert centre.any() and float(centre.max()) < 2.0
        err = np.abs(got.astype(np.float64) - centre.astype(np.float64))
        below = centre < 1.0
        print(f"{name}: largest |rr_albedo_pixels - rr_surface_pixels| {err.max():.3e} over {int(below.sum())} values below 1 and {int((~below).sum())} in [1, 2)")
        assert (err[below] <= 2.0 ** -25).all() and (err[~below] <= 2.0 ** -24).all()


def test_a_shuffled_list_with_duplicates_answers_as_the_whole_frame(hip, oracle):
    c = _case(hip, oracle, "rich", 4)
    rng = np.random.default_rng(5)
    at = rng.integers(0, N, N - 7)                                   # 1893 entries: duplicates, any order, no multiple of 64 / G
    assert len(np.unique(at)) < len(at)
    pixels = np.stack([at % W, at // W], axis=1)
    with hip.DeviceScene(c["fs"], 0) as ds:
        got = ds.albedo_pixels(c["cam"], c["cfg"], pixels=pixels)
        st = ds.stats()
        bad = pixels.copy()
        bad[17] = (W, 3)
        out = np.full((len(bad), 3), 7.0, F)
        xy = hip.pack_pixels(bad)
        rc = hip.lib().rr_albedo_pixels(ds._h, C.byref(c["cam"]), C.byref(c["cfg"]), None, xy.ctypes.data_as(C.c_void_p), len(xy), out.ctypes.data_as(C.c_void_p), None)
        assert rc == -1 and b"pixel_xy[17] = (50, 3) lies outside the frame of 50x38" in hip.lib().rr_last_error() and (out == 7.0).all()
    assert np.array_equal(_bits(got), _bits(c["want"][at]))
    assert st["primary_rays"] == (N - 7) * 4 and st["shaded_hits"] == 0


def test_batches_and_chunks_give_the_same_bytes(hip, oracle):
    """128 samples (243200 primary rays) under a queue budget that makes two batches of 121600 and shade chunks of 65536, two per batch,
    against the default tuning's one batch and one chunk; and 4 samples in batches of 4096 rays against the expected bits."""
    c = _case(hip, oracle, "rich", 4)
    cfg = _cfg(128)
    with hip.DeviceScene(c["fs"], 0) as ds:
        one = ds.albedo_pixels(c["cam"], cfg)
        one_batches = ds.stats()["batches"]
        ds.set_tuning(queue_budget_bytes=128 * 130000, shade_chunk_rays=65536)
        cut = ds.albedo_pixels(c["cam"], cfg)
        cut_batches = ds.stats()["batches"]
        ds.set_tuning(queue_budget_bytes=4096, shade_chunk_rays=65536, sample_group=1)
        small = ds.albedo_pixels(c["cam"], c["cfg"])
        small_batches = ds.stats()["batches"]
    assert one_batches == 1 and cut_batches == 2 and small_batches == 2
    assert np.array_equal(_bits(one), _bits(cut))
    assert np.array_equal(_bits(small), _bits(c["want"]))


def test_device_form_on_a_stream_behind_a_producer(hip, oracle):
    c = _case(hip, oracle, "rich", 4)
    rng = np.random.default_rng(11)
    xy = (rng.integers(0, W, 257) | (rng.integers(0, H, 257) << 16)).astype(np.uint32)
    at = (xy >> 16) * W + (xy & 0xffff)
    with hip.DeviceScene(c["fs"], 0) as ds:
        st = torch.cuda.Stream()
        src = torch.from_numpy(xy.view(np.int32)).cuda()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            whole = renderer.albedo_pixels_torch(ds, c["cam"], c["cfg"])
            listed = renderer.albedo_pixels_torch(ds, c["cam"], c["cfg"], src + 0)        # the list is produced on the stream the call runs on
        st.synchronize()
        host_listed = ds.albedo_pixels(c["cam"], c["cfg"], pixels=xy)
        with pytest.raises(ValueError):
            renderer.albedo_pixels_torch(ds, c["cam"], c["cfg"], src.cpu())
    assert whole.shape == (N, 3) and whole.dtype == torch.float32 and whole.is_cuda
    assert np.array_equal(_bits(whole.cpu().numpy()), _bits(c["got"]))
    assert np.array_equal(_bits(listed.cpu().numpy()), _bits(host_listed)) and np.array_equal(_bits(host_listed), _bits(c["got"][at]))


def test_device_form_refusals_name_their_argument_and_launch_nothing(hip, oracle):
    c = _case(hip, oracle, "rich", 4)
    L, cam, cfg = hip.lib(), c["cam"], c["cfg"]
    with hip.DeviceScene(c["fs"], 0) as ds:
        alb = torch.full((N * 12 + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        xy = torch.zeros((N,), dtype=torch.int32, device="cuda")
        dev = lambda p_xy, p_alb: L.rr_albedo_pixels_device(ds._h, C.byref(cam), C.byref(cfg), None, p_xy, N, p_alb, None, None)
        P = lambda v: C.c_void_p(v)
        assert dev(None, P(alb.data_ptr() + 2)) == -1 and b"rr_albedo_pixels_device" in L.rr_last_error() and b"albedo_out_dev is not 4-byte aligned" in L.rr_last_error()
        assert dev(P(xy.data_ptr() + 1), P(alb.data_ptr())) == -1 and b"pixel_xy_dev is not 4-byte aligned" in L.rr_last_error()
        host = np.zeros(N * 12 + 16, np.uint8)
        ph = host.ctypes.data + (-host.ctypes.data) % 16
        assert dev(None, P(ph)) == -1 and b"albedo_out_dev" in L.rr_last_error() and b"cannot address" in L.rr_last_error()
        assert dev(P(ph), P(alb.data_ptr())) == -1 and b"pixel_xy_dev" in L.rr_last_error() and b"cannot address" in L.rr_last_error()
        # a list entry outside the frame: refused by its index after the call's one wait, nothing written
        xy[1234] = W | (2 << 16)
        torch.cuda.synchronize()
        assert dev(P(xy.data_ptr()), P(alb.data_ptr())) == -1 and b"pixel_xy[1234] = (50, 2) lies outside the frame of 50x38" in L.rr_last_error()
        torch.cuda.synchronize()
        assert (alb.cpu().numpy() == SENTINEL).all() and not host.any()
        # and the handle answers afterwards
        assert dev(None, P(alb.data_ptr())) == 0
        torch.cuda.synchronize()
        assert np.array_equal(alb.cpu().numpy()[:N * 12].view(np.uint32).reshape(N, 3), _bits(c["got"]))


def test_frames_around_the_call_and_a_pixel_query_behind_it(hip, oracle):
    c = _case(hip, oracle, "rich", 4)
    cam = c["cam"]
    cfg = make_config(samples=3, monte_carlo=True, seed=3, max_recursion=4)
    with hip.DeviceScene(c["fs"], 0) as fresh:
        want_pixels = fresh.render_pixels(cam, cfg)
    with hip.DeviceScene(c["fs"], 0) as ds:
        before = ds.render(cam, cfg, aux=True)
        got = ds.albedo_pixels(cam, c["cfg"])
        st = ds.stats()
        pixels = ds.render_pixels(cam, cfg)                          # right after the call: what a fresh handle returns
        listed = ds.albedo_pixels(cam, c["cfg"], pixels=np.array([[1, 2], [40, 30]]))
        after = ds.render(cam, cfg, aux=True)
    assert np.array_equal(_bits(got), _bits(c["got"])) and np.array_equal(_bits(listed), _bits(c["got"][[2 * W + 1, 30 * W + 40]]))
    assert st["primary_rays"] == N * 4 and st["secondary_rays"] == 0 and st["shadow_rays"] == 0 and st["shaded_hits"] == 0
    assert_frames_identical(before, after, "rr_render around rr_albedo_pixels")
    for k in ("color", "depth", "normal", "object_id"):
        assert np.array_equal(np.ascontiguousarray(pixels[k]).view(np.uint32), np.ascontiguousarray(want_pixels[k]).view(np.uint32)), k


def test_refused_from_on_pass_and_cancelled_beforehand(hip, oracle):
    c = _case(hip, oracle, "rich", 4)
    cam = c["cam"]
    seen = []
    with hip.DeviceScene(c["fs"], 0) as ds:
        def on_pass(out, done, total):
            try:
                ds.albedo_pixels(cam, c["cfg"])
                seen.append(None)
            except hip.RustrayHipError as e:
                seen.append((e.code, str(e)))
            return False
        ds.render_progressive(cam, make_config(samples=4, max_recursion=1), on_pass, min_passes=2)
        assert seen and all(s is not None and s[0] == -1 and "rr_albedo_pixels" in s[1] for s in seen), seen
        flag = C.c_int(1)
        with pytest.raises(hip.RustrayHipError) as e:
            ds.albedo_pixels(cam, c["cfg"], cancel=flag)
        assert e.value.code == -6
        alb = torch.full((N, 3), 3.0, dtype=torch.float32, device="cuda")
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            with pytest.raises(hip.RustrayHipError) as e:
                ds.albedo_pixels_device(cam, c["cfg"], None, N, alb.data_ptr(), st.cuda_stream, cancel=flag)
        assert e.value.code == -6 and st.query()                       # the stream is idle when the call returns
        # the handle answers afterwards
        assert np.array_equal(_bits(ds.albedo_pixels(cam, c["cfg"])), _bits(c["got"]))
