"""rr_render_pixel_split on the GPU, every comparison bit for bit and over every pixel and channel.

THE TOTAL: out and halves are render_pixel_parts' at n_parts = 2 (render_pixels' without halves).
THE DIFFUSE TERM: diffuse and diffuse_halves are the colour and the halves render_pixel_parts returns for an EDITED COPY of the scene --
every material's ambient_color and specular_color 0 -- under fog_color (0, 0, 0) at the same density and max_recursion 0.  Why they are
equal: 0 * light_power + x is x, so a light's term of the copy is the frame's term without its specular product; the constant term is
thr * (0 * fa + 0) = 0; nothing spawns at recursion 0; w_light reads none of the edited fields; and a_mul is the same at recursion 0 and
4 unless a primary hit is totally internally reflected: k < 0 needs eta > 1, which a front-face hit has with refraction_index < 1 and a
BACK-face hit (the camera looks at the inside of a surface) with refraction_index > 1.  So every material whose alpha can be below 1 is
checked on the CPU below and gets index 1 (eta = 1: k = i_dot_n^2 >= 0) in the copy both frames are made from.  The shadow ray of a light is the same ray in both frames (origin, jittered direction and
generator key do not read the edited fields) and is traced in the copy whenever the diffuse term is not zero.

Frames of 50x38 (a partial last packet) of rich_scene(9119) (20 items: packet top level, fixed shadow slots, every map), spheres_room
(14 items: the dense level-1 queue) and the checkered floor; a scene of a floor that takes no shadows under 40 lights for the 32-light
flush (and, one light being strong, for the terms beyond 2 that take the 64-bit path)."""
import copy
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from rustray_amd import renderer
from rustray_amd.flat import FlatScene, Item, Light, Material, make_config
from tests.helpers import camera_for, load_scene
from tests.test_gpu_denoise_albedo import _checkered_floor

pytestmark = pytest.mark.gpu

W, H = 50, 38
N = W * H
F = np.float32
SENTINEL = 0x5a5a5a5a
SCENES = ("rich", "spheres_room", "floor", "forty_lights")
CONFIGS = ("plain4", "dof8", "table4")
_scenes = {}
_cache = {}


def _forty_lights():
    """A floor that takes no shadows and a ball that does, under 40 point lights on a ring (one of them strong): the floor's light terms
    are added directly, flushed at the 32nd light; the ball's go through the dense shadow queue (more than 32 lights: no fixed slots)."""
    from tests import corner_scenes as cs
    fs = FlatScene()
    fs.meshes = [cs._quad(0.0, 5.0)]
    cs._mesh_item(fs, 0, Material(base_color=(0.8, 0.6, 0.4), ambient_color=(0.05, 0.05, 0.1), specular_color=(0.6, 0.6, 0.6), shininess=20.0, receive_shadow=False), 3,
                  "floor")
    mi, ci = cs._mat(fs, Material(base_color=(0.3, 0.6, 0.9), ambient_color=(0.02, 0.02, 0.02), shininess=40.0, reflectivity=0.3))
    t = cs.EYE.copy(); t[:3, 3] = (0.0, 1.0, 0.0); ti = cs.EYE.copy(); ti[:3, 3] = (0.0, -1.0, 0.0)
    fs.items.append(Item(kind=0, id=6, material=mi, material_cache=ci, radius=1.0, trans=t, trans_inv=ti, bbox_min=(-1.0,) * 3, bbox_max=(1.0,) * 3, name="ball"))
    fs.lights = [Light(pos=(4.0 * float(np.cos(k * 0.157)), 3.0 + 0.05 * k, 4.0 * float(np.sin(k * 0.157))), color=(1.0, 0.9 - 0.01 * k, 0.5 + 0.01 * k),
                       intensity=3000.0 if k == 5 else 6.0) for k in range(40)]
    cs._cam(fs, eye=(0.0, 4.0, 7.0), direction=(0.0, -0.5, -1.0))
    return fs


def _scene(name):
    """The scene both frames are made from, checked on the CPU for what the comparison needs (see the module's text)."""
    if name not in _scenes:
        if name == "rich":
            from tools.fuzz_parity import rich_scene
            fs = rich_scene(9119)
        elif name == "floor":
            fs = _checkered_floor()
        elif name == "forty_lights":
            fs = _forty_lights()
        else:
            fs = load_scene(name)
        fs = _with_materials(fs, [dataclasses.replace(m, texture=list(m.texture)) for m in fs.materials])
        fixed = 0
        for m in fs.materials:
            assert np.isfinite(m.shininess) and m.shininess >= 0.0
            if m.refraction_index != 1.0 and (m.alpha < 1.0 or m.texture[0] >= 0 or m.texture[4] >= 0):    # alpha may come from a map
                m.refraction_index, fixed = 1.0, fixed + 1
        if fixed:
            print(f"{name}: {fixed} materials whose alpha can be below 1 had a refraction_index other than 1 and got index 1")
        _scenes[name] = fs
    return _scenes[name]


def _with_materials(fs, materials):
    """`fs` with other materials: a scene of its own that shares the meshes, textures, items and lights."""
    out = FlatScene()
    out.items, out.meshes, out.textures, out.lights = list(fs.items), list(fs.meshes), list(fs.textures), list(fs.lights)
    out.name, out.meta = fs.name, copy.deepcopy(fs.meta)
    out.materials = materials
    return out


def _diffuse_only(fs):
    return _with_materials(fs, [dataclasses.replace(m, ambient_color=(0.0, 0.0, 0.0), specular_color=(0.0, 0.0, 0.0), texture=list(m.texture)) for m in fs.materials])


def _cfg(config, samples=None, reference=False):
    kw = dict(plain4=dict(samples=4, max_recursion=4, seed=5),
              dof8=dict(samples=8, max_recursion=4, seed=77, monte_carlo=True, fog_density=0.02, focal_length=4.0, aperture_size=2.5),
              table4=dict(samples=4, max_recursion=4, seed=9, monte_carlo=True))[config]
    if samples:
        kw["samples"] = samples
    if reference:     # the frame of the edited copy: black fog at the same density, nothing spawns
        kw.update(fog_color=(0.0, 0.0, 0.0), max_recursion=0)
    return make_config(**kw)


def _table(hip, config, samples):
    if config != "table4":
        return None
    table, _ = hip.sample_table(samples)      # a caller's table: every cell of the built-in one mirrored, in reverse order
    table = np.ascontiguousarray(table, np.uint16).reshape(samples, 2)
    return np.ascontiguousarray((int(table.max()) - table)[::-1])


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _case(hip, name, config):
    """One scene at one config, computed once and left unchanged: the split call's whole-frame answer, render_pixel_parts' for the same
    arguments, and render_pixel_parts' colours for the edited copy."""
    key = (name, config)
    if key not in _cache:
        fs = _scene(name)
        cam = camera_for(fs, W, H).c_struct()
        cfg = _cfg(config)
        table = _table(hip, config, cfg.samples)
        with hip.DeviceScene(fs, 0) as ds:
            before = ds.render_pixels(cam, cfg, sample_xy=table)
            got = ds.render_pixel_split(cam, cfg, sample_xy=table); got_stats = ds.stats()
            after = ds.render_pixels(cam, cfg, sample_xy=table)
            want = ds.render_pixel_parts(cam, cfg, n_parts=2, sample_xy=table); want_stats = ds.stats()
        with hip.DeviceScene(_diffuse_only(fs), 0) as ds:
            ref = ds.render_pixel_parts(cam, _cfg(config, reference=True), n_parts=2, sample_xy=table)
        _cache[key] = dict(fs=fs, cam=cam, cfg=cfg, table=table, got=got, want=want, ref=ref, before=before, after=after, got_stats=got_stats, want_stats=want_stats)
    return _cache[key]


def _differ(got, want, what):
    d = _bits(got) != _bits(want)
    assert got.shape == want.shape and not d.any(), (f"{what}: {int(d.sum())} of {d.size} words differ, the first at {np.argwhere(d)[0].tolist()}: "
                                                      f"got {np.asarray(got)[tuple(np.argwhere(d)[0])]!r}, want {np.asarray(want)[tuple(np.argwhere(d)[0])]!r}")


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("name", SCENES)
def test_the_total_is_render_pixel_parts(hip, name, config):
    c = _case(hip, name, config)
    got, want = c["got"], c["want"]
    for k in ("color", "depth", "normal", "object_id"):
        _differ(got[k], want[k], f"out.{k}")
        _differ(got["parts"][k], want["parts"][k], f"halves.{k}")
    assert got["color"].shape == (N, 3) and got["parts"]["color"].shape == (N, 2, 3) and got["diffuse"].shape == (N, 3) and got["diffuse_halves"].shape == (N, 2, 3)
    # the counters are those of the parts call for the same frame
    for k in ("primary_rays", "secondary_rays", "shadow_rays", "shaded_hits", "batches"):
        assert c["got_stats"][k] == c["want_stats"][k], k
    assert c["got_stats"]["primary_rays"] == N * c["cfg"].samples and c["got_stats"]["shadow_rays"] > 0
    # a render_pixels call before the split call and one after it return identical bytes
    for k in ("color", "depth", "normal", "object_id"):
        _differ(c["after"][k], c["before"][k], f"render_pixels around the call, {k}")
        _differ(c["before"][k], got[k], f"render_pixels against out.{k}")


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("name", SCENES)
def test_the_diffuse_term_is_the_frame_of_the_edited_copy(hip, name, config):
    c = _case(hip, name, config)
    got, ref = c["got"], c["ref"]
    assert np.isfinite(got["color"]).all() and np.isfinite(got["parts"]["color"]).all()          # the condition of the comparison
    assert np.isfinite(ref["color"]).all() and ref["color"].any()
    _differ(got["diffuse"], ref["color"], "diffuse")
    _differ(got["diffuse_halves"], ref["parts"]["color"], "diffuse_halves")
    # it is a part of the colour, and a proper one: something is left for `rest` (ambient, fog, highlights, what spawns)
    # (a light's term is not below its diffuse part -- rounding is monotone -- so only the two conversions to binary32 can make rest negative)
    rest = got["color"].astype(np.float64) - got["diffuse"]
    assert (rest >= -2.0 ** -22 * np.maximum(1.0, got["color"])).all() and (rest > 1e-3).any()
    if name == "forty_lights":      # the strong light's terms are beyond 2: the 64-bit path of fix_add
        assert float(got["diffuse"].max()) * c["cfg"].samples > 2.0


@pytest.mark.parametrize("name", SCENES)
def test_three_samples_without_halves_is_render_pixels(hip, name):
    fs = _scene(name)
    cam = camera_for(fs, W, H).c_struct()
    cfg = _cfg("plain4", samples=3)
    with hip.DeviceScene(fs, 0) as ds:
        got = ds.render_pixel_split(cam, cfg, halves=False)
        want = ds.render_pixels(cam, cfg)
        with pytest.raises(hip.RustrayHipError) as e:        # halves need an even count: the parts call's refusal
            ds.render_pixel_split(cam, cfg)
        assert e.value.code == -1 and "n_parts 2 does not divide samples 3" in str(e.value)
    with hip.DeviceScene(_diffuse_only(fs), 0) as ds:
        ref = ds.render_pixels(cam, _cfg("plain4", samples=3, reference=True))
    assert "parts" not in got and "diffuse_halves" not in got
    for k in ("color", "depth", "normal", "object_id"):
        _differ(got[k], want[k], f"out.{k}")
    _differ(got["diffuse"], ref["color"], "diffuse")


def test_a_list_gives_the_rows_of_the_whole_frame(hip):
    c = _case(hip, "rich", "dof8")
    rng = np.random.default_rng(5)
    at = rng.integers(0, N, N - 7)                                   # 1893 entries: duplicates, any order, no multiple of 64 / G
    pixels = np.stack([at % W, at // W], axis=1)
    with hip.DeviceScene(c["fs"], 0) as ds:
        got = ds.render_pixel_split(c["cam"], c["cfg"], pixels=pixels)
        assert ds.stats()["primary_rays"] == (N - 7) * c["cfg"].samples
        bad = pixels.copy()
        bad[17] = (W, 3)
        with pytest.raises(hip.RustrayHipError) as e:
            ds.render_pixel_split(c["cam"], c["cfg"], pixels=bad)
        assert e.value.code == -1 and "pixel_xy[17] = (50, 3) lies outside the frame of 50x38" in str(e.value)
        assert ds.render_pixel_split(c["cam"], c["cfg"], pixels=np.zeros((0, 2), np.int64))["diffuse"].shape == (0, 3)     # n_pixels == 0: RR_OK
    whole = c["got"]
    for k in ("color", "depth", "normal", "object_id"):
        _differ(got[k], whole[k][at], f"out.{k}")
        _differ(got["parts"][k], whole["parts"][k][at], f"halves.{k}")
    _differ(got["diffuse"], whole["diffuse"][at], "diffuse")
    _differ(got["diffuse_halves"], whole["diffuse_halves"][at], "diffuse_halves")


def test_batches_and_chunks_give_the_same_bytes(hip):
    """The frame in several batches and shade chunks (a small queue budget, sample groups of one) holds the bits of the default plan."""
    for name in ("rich", "spheres_room"):
        c = _case(hip, name, "dof8")
        with hip.DeviceScene(c["fs"], 0) as ds:
            ds.set_tuning(queue_budget_bytes=4096, sample_group=1)          # batches of 4096 primary rays at most: one sample slice of 3800 each
            got = ds.render_pixel_split(c["cam"], c["cfg"])
            assert ds.stats()["batches"] > 1
        for k in ("color", "diffuse", "diffuse_halves"):
            _differ(got[k], c["got"][k], f"{name} {k}")
        _differ(got["parts"]["color"], c["got"]["parts"]["color"], f"{name} halves.color")


def test_device_form_on_a_stream_behind_a_producer(hip):
    c = _case(hip, "rich", "plain4")
    rng = np.random.default_rng(11)
    xy = (rng.integers(0, W, 257) | (rng.integers(0, H, 257) << 16)).astype(np.uint32)
    at = (xy >> 16) * W + (xy & 0xffff)
    with hip.DeviceScene(c["fs"], 0) as ds:
        st = torch.cuda.Stream()
        src = torch.from_numpy(xy.view(np.int32)).cuda()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            whole = renderer.render_pixel_split_torch(ds, c["cam"], c["cfg"])
            listed = renderer.render_pixel_split_torch(ds, c["cam"], c["cfg"], src + 0)          # the list is produced on the stream the call runs on
            plain = renderer.render_pixel_split_torch(ds, c["cam"], c["cfg"], halves=False)
        st.synchronize()
        with pytest.raises(ValueError):
            renderer.render_pixel_split_torch(ds, c["cam"], c["cfg"], src.cpu())
    g = c["got"]
    rec = whole["records"].cpu().numpy()
    assert whole["diffuse"].is_cuda and rec.shape == (N, 8)
    _differ(rec[:, 0:3], g["color"], "whole frame, colour")
    _differ(whole["part_records"].cpu().numpy()[:, :, 0:3], g["parts"]["color"], "whole frame, halves")
    _differ(whole["diffuse"].cpu().numpy(), g["diffuse"], "whole frame, diffuse")
    _differ(whole["diffuse_halves"].cpu().numpy(), g["diffuse_halves"], "whole frame, diffuse halves")
    _differ(listed["records"].cpu().numpy()[:, 0:3], g["color"][at], "list, colour")
    _differ(listed["diffuse"].cpu().numpy(), g["diffuse"][at], "list, diffuse")
    _differ(listed["diffuse_halves"].cpu().numpy(), g["diffuse_halves"][at], "list, diffuse halves")
    assert "part_records" not in plain and "diffuse_halves" not in plain
    _differ(plain["records"].cpu().numpy()[:, 0:3], g["color"], "no halves, colour")
    _differ(plain["diffuse"].cpu().numpy(), g["diffuse"], "no halves, diffuse")


def test_refusals_name_their_argument_and_write_nothing(hip):
    c = _case(hip, "rich", "plain4")
    L, cam, cfg = hip.lib(), c["cam"], c["cfg"]
    odd = _cfg("plain4", samples=3)
    P = lambda v: C.c_void_p(v)
    err = L.rr_last_error
    with hip.DeviceScene(c["fs"], 0) as ds:
        out = torch.full((N * 8 + 16,), SENTINEL, dtype=torch.int32, device="cuda")
        hv = torch.full((N * 16 + 16,), SENTINEL, dtype=torch.int32, device="cuda")
        dif = torch.full((N * 3 + 16,), SENTINEL, dtype=torch.int32, device="cuda")
        dh = torch.full((N * 6 + 16,), SENTINEL, dtype=torch.int32, device="cuda")
        o, h, d, e = out.data_ptr(), hv.data_ptr(), dif.data_ptr(), dh.data_ptr()
        dev = lambda po, ph, pd, pe, cf=cfg, n=N: L.rr_render_pixel_split_device(ds._h, C.byref(cam), C.byref(cf), None, None, n, P(po), P(ph), P(pd), P(pe), None, None)
        host = lambda po, ph, pd, pe, cf=cfg: L.rr_render_pixel_split(ds._h, C.byref(cam), C.byref(cf), None, None, N, P(po), P(ph), P(pd), P(pe), None)
        hb = np.full(N * 16 + 8, 7.0, F)
        hp = hb.ctypes.data + (-hb.ctypes.data) % 16
        for fn, name in ((dev, b"rr_render_pixel_split_device"), (host, b"rr_render_pixel_split")):
            a = (o, h, d, e) if fn is dev else (hp, hp, hp, hp)        # (the host form refuses before it looks at where the pointers lead)
            assert fn(None, a[1], a[2], a[3]) == -1 and name in err() and b"out is required" in err()
            assert fn(a[0], a[1], None, a[3]) == -1 and b"diffuse_out is required" in err()
            assert fn(a[0], a[1], a[2], None) == -1 and b"given together or not at all" in err()
            assert fn(a[0], None, a[2], a[3]) == -1 and b"given together or not at all" in err()
            assert fn(a[0], a[1], a[2], a[3], odd) == -1 and b"n_parts 2 does not divide samples 3" in err()
        assert dev(o, h, d, e, cfg, 7) == -1 and b"7 pixels without a list" in err()
        assert dev(o + 8, h, d, e) == -1 and b"must be 16-byte aligned" in err()
        assert dev(o, h + 4, d, e) == -1 and b"must be 16-byte aligned" in err()
        assert dev(o, h, d + 2, e) == -1 and b"must be 4-byte aligned" in err()
        assert dev(o, h, d, e + 1) == -1 and b"must be 4-byte aligned" in err()
        assert dev(o, h, d, d + 4 * 3 * (N - 1)) == -1 and b"overlaps" in err()
        assert dev(o, h, hp, e) == -1 and b"diffuse_out_dev" in err() and b"cannot address" in err()
        torch.cuda.synchronize()
        for t in (out, hv, dif, dh):
            assert (t.cpu().numpy().view(np.uint32) == SENTINEL).all()
        assert (hb == 7.0).all()
        # and the handle answers afterwards, writing exactly its outputs
        assert dev(o, h, d, e) == 0
        torch.cuda.synchronize()
        g = c["got"]
        _differ(out.cpu().numpy()[:N * 8].view(F).reshape(N, 8)[:, 0:3], g["color"], "out")
        _differ(dif.cpu().numpy()[:N * 3].view(F).reshape(N, 3), g["diffuse"], "diffuse")
        _differ(dh.cpu().numpy()[:N * 6].view(F).reshape(N, 2, 3), g["diffuse_halves"], "diffuse halves")
        for t, n in ((out, N * 8), (hv, N * 16), (dif, N * 3), (dh, N * 6)):
            assert (t.cpu().numpy()[n:].view(np.uint32) == SENTINEL).all()


def test_refused_from_on_pass_and_cancelled_beforehand(hip):
    c = _case(hip, "rich", "plain4")
    cam = c["cam"]
    seen = []
    with hip.DeviceScene(c["fs"], 0) as ds:
        def on_pass(out, done, total):
            try:
                ds.render_pixel_split(cam, c["cfg"])
                seen.append(None)
            except hip.RustrayHipError as e:
                seen.append((e.code, str(e)))
            return False
        ds.render_progressive(cam, make_config(samples=4, max_recursion=1), on_pass, min_passes=2)
        assert seen and all(s is not None and s[0] == -1 and "rr_render_pixel_split" in s[1] for s in seen), seen
        flag = C.c_int(1)
        with pytest.raises(hip.RustrayHipError) as e:
            ds.render_pixel_split(cam, c["cfg"], cancel=flag)
        assert e.value.code == -6
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            out = torch.zeros((N, 8), dtype=torch.float32, device="cuda")
            dif = torch.zeros((N, 3), dtype=torch.float32, device="cuda")
            with pytest.raises(hip.RustrayHipError) as e:
                ds.render_pixel_split_device(cam, c["cfg"], None, N, out.data_ptr(), None, dif.data_ptr(), None, st.cuda_stream, cancel=flag)
        assert e.value.code == -6 and st.query()                       # the stream is idle when the call returns
        got = ds.render_pixel_split(cam, c["cfg"])                     # the handle answers afterwards
    _differ(got["diffuse"], c["got"]["diffuse"], "after a cancelled call")
    _differ(got["color"], c["got"]["color"], "after a cancelled call")


def test_cpp_render_pixel_split(hip):
    from tests.test_cpp_host import _cam_args
    from tests.test_gpu_pixel_parts_cpp import _shim
    c = _case(hip, "rich", "plain4")
    L = _shim()
    cam_types = list(L.rh_render_pixel_parts.argtypes[1:10])
    L.rh_render_pixel_split.argtypes = [C.c_void_p] + cam_types + [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    cs = c["fs"].c_struct()
    h = L.rh_scene_create(C.byref(cs), 0)
    assert h
    try:
        args = _cam_args(camera_for(c["fs"], W, H)) + (C.byref(c["cfg"]), W, H)
        out, hv, dif, dh = np.zeros((N, 8), F), np.zeros((N, 2, 8), F), np.zeros((N, 3), F), np.zeros((N, 2, 3), F)
        assert L.rh_render_pixel_split(h, *args, None, 0, out.ctypes.data, hv.ctypes.data, dif.ctypes.data, dh.ctypes.data) == N
        assert L.rh_render_pixel_split(h, *args, None, 0, out.ctypes.data, hv.ctypes.data, dif.ctypes.data, None) == -1     # halves without diffuse halves
    finally:
        L.rh_scene_destroy(h)
    g = c["got"]
    _differ(out[:, 0:3], g["color"], "out")
    _differ(hv[:, :, 0:3], g["parts"]["color"], "halves")
    _differ(dif, g["diffuse"], "diffuse")
    _differ(dh, g["diffuse_halves"], "diffuse halves")
