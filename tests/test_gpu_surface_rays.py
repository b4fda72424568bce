"""rr_surface_rays: position, normals, uv and material of the closest hits of caller-supplied rays, against the oracle.

The rays are the oracle's own primaries (rro_primary_ray) of a 50 x 38 frame at 1 sample, in row-major pixel order, with the
direction normalised in numpy float32 the way get_color_depth_normal_id normalises it on entry (d / sqrt((x x + y y) + z z)): 1 900
rays, seven full workgroups and a 108-ray tail with a partial wave.  Ray y * w + x is then that frame's pixel, and the judge is the
oracle's float64 means of a 1-sample frame with monte_carlo = 0, max_recursion = 0, no fog and no lights: the colour of a hit is then
exactly its ambient colour, and mean_depth / mean_normal are the sample's own f32 values.  The other colours and the scalar maps are
read through PROBE VARIANTS that only the oracle renders: a copy of the scene whose every material has ambient_color := the colour
in question (or (1, 1, 1)) and texture[AMBIENT] := texture[that slot], so that the frame's colour is the value itself.  The query
runs once per scene, on the unedited scene.

Float comparisons use the project's band, e = BAND_EPS_REL |m| + BAND_EPS_ABS (tests/helpers.py), with nothing left out; bit equality
is expected and counted, not gated.  One MI355X, worst |err| / e and words that are not bit-equal, per field:

    normal, ambient_color, base_color.xyz, specular_color (3 x 5 700 words each): 0.0000, every word bit-equal, on all three scenes
    ambient_occlusion (52 hits with the map), reflectivity (53), rich scene:      0.0000, every word bit-equal
    alpha / (material.alpha * base_color.w) against the alpha texel (89 hits):    0.0033 (a quotient: bit equality does not apply)
    roughness * 2 PI against the roughness texel (244 hits):                      0.0081 (likewise)
    shading_normal against the float64 restatement (79 normal-mapped hits):       worst |err| 8.443e-08 = 2^-23.50, bound 2^-18
    uv: 255 nearest-filter textured hits re-sample their texels to the bit
    (spheres_room and monkey carry no maps: their scalar fields are the plain material values, bit for bit.)
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from rustray_amd import renderer
from rustray_amd.flat import SURFACE_HIT_DTYPE, make_config
from tests.helpers import BAND_EPS_ABS, BAND_EPS_REL, assert_frames_identical, camera_for, load_scene
from tests.test_gpu_shade_rays import primaries

pytestmark = pytest.mark.gpu

W, H = 50, 38
N = W * H
SCENES = ("rich", "spheres_room", "monkey")
HITS = dict(rich=430, spheres_room=1900, monkey=160)
BASE, AMBIENT, SPECULAR, NORMAL, ALPHA, ROUGHNESS, AO, REFLECTIVITY = range(8)   # TextureType order
SENTINEL = 0x5a5a5a5a
_cache = {}


def _scene(name):
    if name == "rich":
        from tools.fuzz_parity import rich_scene   # 20 items (packet top level), every texture slot, nearest and bilinear, flipped normals
        return rich_scene(9119)
    return load_scene(name)                        # spheres_room: 14 items, the per-ray walk, smooth meshes; monkey: one untextured mesh


def _cfg():
    return make_config(samples=1, monte_carlo=False, seed=3, max_recursion=0, fog_density=0.0)


def _probe(fs, colour=None, slot=None):
    """The light-less copy of `fs`; with `colour` ("base_color", "specular_color") or `slot` (3 .. 7): every material's ambient colour
    := that colour (or (1, 1, 1)) and texture[AMBIENT] := texture[slot]."""
    out = copy.deepcopy(fs)
    out.lights = []
    if colour is None and slot is None:
        return out
    for m in out.materials:
        m.ambient_color = tuple(getattr(m, colour)) if colour else (1.0, 1.0, 1.0)
        m.texture = list(m.texture)
        m.texture[AMBIENT] = m.texture[slot]
    return out


def _f32_normalised(d):
    d = np.ascontiguousarray(d, np.float32)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    n = np.sqrt((x * x + y * y) + z * z)
    assert n.dtype == np.float32
    return np.ascontiguousarray(d / n[:, None])


def _rays_and_refs(oracle, name):
    """What needs no GPU: the rays and the oracle's frames of the scene's probe variants (the means are float64 of f32 values)."""
    fs = _scene(name)
    cam = camera_for(fs, W, H).c_struct()
    cfg = _cfg()
    table, _ = oracle.sample_table(1)
    o, d = primaries(oracle, cam, cfg, table)
    d = _f32_normalised(d)
    variants = {"ambient": _probe(fs), "base": _probe(fs, "base_color", BASE), "specular": _probe(fs, "specular_color", SPECULAR)}
    variants.update({s: _probe(fs, None, s) for s in (NORMAL, ALPHA, ROUGHNESS, AO, REFLECTIVITY)})
    ref = {k: oracle.render(v.c_struct(), cam, cfg, sample_xy=table, want_means=True, n_threads=8) for k, v in variants.items()}
    for k, r in ref.items():   # the judge is finite everywhere, f32-exact, and every variant sees the same hits
        for f in ("mean_rgb", "mean_depth", "mean_normal"):
            assert np.isfinite(r[f]).all(), (name, k, f)
            assert np.array_equal(r[f], r[f].astype(np.float32).astype(np.float64)), (name, k, f)
        assert np.array_equal(r["object_id"], ref["ambient"]["object_id"]) and np.array_equal(r["mean_depth"], ref["ambient"]["mean_depth"]), (name, k)
    return dict(fs=fs, cam=cam, cfg=cfg, table=table, o=o, d=d, ref=ref)


def _raw_hits(hip, ds, o, d, depth=1):
    out = np.full((len(o), 5), SENTINEL, np.uint32)
    hip._check(hip.lib().rr_trace_rays(ds._h, o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p), len(o), depth, out.ctypes.data_as(C.c_void_p)))
    return out


def _case(hip, oracle, name):
    if name not in _cache:
        c = _rays_and_refs(oracle, name)
        with hip.DeviceScene(c["fs"], 0) as ds:
            c["got"] = ds.surface_rays(c["o"], c["d"], 1)
            c["hits"] = _raw_hits(hip, ds, c["o"], c["d"])
        c["got"].setflags(write=False)
        g = c["got"]
        c["hit"] = g["hit"] == 1
        c["mat"] = [c["fs"].materials[c["fs"].items[int(i)].material] if h else None for i, h in zip(g["item_index"], c["hit"])]
        _cache[name] = c
    return _cache[name]


def _bytes(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(len(a), a.dtype.itemsize * int(np.prod(a.shape[1:])))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _has(c, slot):
    """Per ray: a hit whose material carries a map in `slot`."""
    return np.array([m is not None and m.texture[slot] >= 0 for m in c["mat"]], bool)


def _in_band(what, got, m, where=None):
    """|got - m| <= BAND_EPS_REL |m| + BAND_EPS_ABS on every element (of the rows `where`); prints the worst |err| / e."""
    got = np.asarray(got, np.float64); m = np.asarray(m, np.float64)
    if where is not None:
        got, m = got[where], m[where]
    assert np.isfinite(got).all() and np.isfinite(m).all(), what
    e = BAND_EPS_REL * np.abs(m) + BAND_EPS_ABS
    err = np.abs(got - m)
    worst = float((err / e).max()) if err.size else 0.0
    print(f"surface_rays {what}: {err.size} words, worst |err| / e = {worst:.4f}")
    assert (err <= e).all(), f"{what}: {int((err > e).sum())} of {err.size} outside the band, worst |err| / e = {worst:.4f}"
    return worst


def _direct(what, got32, m):
    """A field the oracle reports itself: in the band everywhere, and the count of words that are not bit-equal to f32(m)."""
    nb = int((_bits(got32) != _bits(np.asarray(m, np.float64).astype(np.float32))).sum())
    print(f"surface_rays {what}: {nb} of {np.asarray(got32).size} words not bit-equal")
    return _in_band(what, got32, m), nb


# ---- 1: identity with the closest-hit query ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_first_row_and_distance_are_rr_trace_rays(hip, oracle, name):
    c = _case(hip, oracle, name)
    g, h = c["got"], c["hits"]
    assert g.dtype == SURFACE_HIT_DTYPE and g.shape == (N,)
    assert int(c["hit"].sum()) == HITS[name]
    for k, f in enumerate(("hit", "item_index", "object_id", "face_id")):
        assert np.array_equal(g[f], h[:, k]), f
    assert np.array_equal(_bits(g["distance"]), h[:, 4])


# ---- 2, 3: depth and position -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_depth_and_position(hip, oracle, name):
    c = _case(hip, oracle, name)
    g, ref = c["got"], c["ref"]["ambient"]
    assert np.array_equal(g["object_id"], ref["object_id"].reshape(N))
    assert np.array_equal(_bits(g["distance"]), _bits(ref["mean_depth"].reshape(N).astype(np.float32)))
    want = c["o"] + c["d"] * g["distance"][:, None]
    assert want.dtype == np.float32
    k = c["hit"]
    assert np.array_equal(_bits(g["position"][k]), _bits(want[k]))


# ---- 4, 5, 6: normal, colours and scalar maps against the oracle's means ------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_normal_and_colours(hip, oracle, name):
    c = _case(hip, oracle, name)
    g, ref = c["got"], c["ref"]
    _direct(f"{name} normal", g["normal"], ref["ambient"]["mean_normal"].reshape(N, 3))
    _direct(f"{name} ambient_color", g["ambient_color"], ref["ambient"]["mean_rgb"].reshape(N, 3))
    _direct(f"{name} base_color.xyz", g["base_color"][:, :3], ref["base"]["mean_rgb"].reshape(N, 3))
    _direct(f"{name} specular_color", g["specular_color"], ref["specular"]["mean_rgb"].reshape(N, 3))


@pytest.mark.parametrize("name", SCENES)
def test_scalar_maps(hip, oracle, name):
    """With the map: the oracle-pinned texel's .x, in the band.  Without: the plain material value, bit for bit."""
    c = _case(hip, oracle, name)
    g, ref, hit = c["got"], c["ref"], c["hit"]
    tx = {s: ref[s]["mean_rgb"].reshape(N, 3)[:, 0] for s in (ALPHA, ROUGHNESS, AO, REFLECTIVITY)}
    mat_f = lambda f: np.array([np.float32(getattr(m, f)) if m is not None else np.float32(0) for m in c["mat"]], np.float32)
    # alpha = material.alpha * base_color.w [* texel.x]
    plain = mat_f("alpha") * g["base_color"][:, 3]
    assert plain.dtype == np.float32
    k = _has(c, ALPHA)
    den = plain.astype(np.float64)
    nz = k & (den != 0.0)
    _in_band(f"{name} alpha / (material.alpha * base_color.w)", g["alpha"][nz].astype(np.float64) / den[nz], tx[ALPHA][nz])
    assert (g["alpha"][k & ~nz] == 0.0).all()   # a zero factor: the quotient does not exist, the product is exactly zero
    assert np.array_equal(_bits(g["alpha"][hit & ~k]), _bits(plain[hit & ~k]))
    # roughness = (1 / PI / 2) * texel.x
    k = _has(c, ROUGHNESS)
    _in_band(f"{name} roughness * 2 PI", g["roughness"][k].astype(np.float64) * (2.0 * np.pi), tx[ROUGHNESS][k])
    assert np.array_equal(_bits(g["roughness"][hit & ~k]), _bits(mat_f("roughness")[hit & ~k]))
    k = _has(c, AO)
    _direct(f"{name} ambient_occlusion", g["ambient_occlusion"][k], tx[AO][k])
    assert (g["ambient_occlusion"][hit & ~k] == 1.0).all()
    k = _has(c, REFLECTIVITY)
    _direct(f"{name} reflectivity", g["reflectivity"][k], tx[REFLECTIVITY][k])
    assert np.array_equal(_bits(g["reflectivity"][hit & ~k]), _bits(mat_f("reflectivity")[hit & ~k]))
    if name == "rich":   # every slot is exercised: hits whose material carries a map, per slot (the ambient slot has the fewest)
        assert [int(_has(c, s).sum()) for s in range(8)] == [332, 36, 294, 79, 89, 244, 52, 53]


# ---- 7: uv ------------------------------------------------------------------------------------------------------------------------
def _tex_wrap(val, bound):
    """tex_wrap: f32 product, cast toward zero, remainder made non-negative."""
    x = np.float32(val) * np.float32(bound)
    assert abs(float(x)) < 2.0 ** 31
    return int(np.trunc(x)) % int(bound)


@pytest.mark.parametrize("name", ("rich",))
def test_uv_gives_the_texels_of_nearest_filter_materials(hip, oracle, name):
    c = _case(hip, oracle, name)
    g, fs = c["got"], c["fs"]
    lut = (np.arange(256, dtype=np.float32) / np.float32(255.0)).astype(np.float32)
    checked = 0
    for i in np.flatnonzero(c["hit"]):
        m = c["mat"][i]
        if not m.texture_filtering_nearest or not any(m.texture[s] >= 0 for s in (BASE, AMBIENT, SPECULAR)):
            continue
        assert g["has_uv"][i] == 1
        u, v = g["uv"][i]
        for slot, field, colour in ((BASE, "base_color", m.base_color), (AMBIENT, "ambient_color", m.ambient_color), (SPECULAR, "specular_color", m.specular_color)):
            if m.texture[slot] < 0:
                continue
            t = fs.textures[m.texture[slot]]
            p = t[_tex_wrap(v, t.shape[0]), _tex_wrap(u, t.shape[1])]
            want = np.array([np.float32(x) for x in colour], np.float32) * lut[p[:3]]
            assert np.array_equal(_bits(g[field][i][:3]), _bits(want)), (i, field)
            if slot == BASE:
                assert _bits(g[field][i][3:4])[0] == _bits(np.float32(1.0) * lut[p[3:4]])[0], (i, "base_color.w")
        checked += 1
    print(f"surface_rays {name} uv: {checked} nearest-filter textured hits re-sampled")
    assert checked >= 32


# ---- 8: shading normal ------------------------------------------------------------------------------------------------------------
def _normal_mapped(n, tc, strength):
    """raytracing.rs:760-783 in float64."""
    unit = lambda a: a / np.sqrt((a * a).sum())
    tangent = np.cross(n, (0.0, 1.0, 0.0))
    if np.sqrt((tangent * tangent).sum()) <= 0.0001:
        tangent = np.cross(n, (0.0, 0.0, 1.0))
    tangent = unit(tangent)
    bitangent = unit(np.cross(n, tangent))
    nm = tc * 2.0 - 1.0
    nm[0] *= strength; nm[1] *= strength
    nm = unit(nm)
    return unit(tangent * nm[0] + bitangent * nm[1] + n * nm[2])


@pytest.mark.parametrize("name", SCENES)
def test_shading_normal(hip, oracle, name):
    """Tolerance 2^-18 per component: fewer than 64 f32 roundings of at most 2^-24 on quantities no larger than 1."""
    c = _case(hip, oracle, name)
    g = c["got"]
    k = _has(c, NORMAL)
    assert np.array_equal(_bits(g["shading_normal"][~k]), _bits(g["normal"][~k]))
    texel = c["ref"][NORMAL]["mean_rgb"].reshape(N, 3)
    worst = 0.0
    for i in np.flatnonzero(k):
        want = _normal_mapped(g["normal"][i].astype(np.float64), texel[i].copy(), float(np.float32(c["mat"][i].normal_map_strength)))
        assert np.isfinite(want).all() and np.isfinite(g["shading_normal"][i]).all()
        worst = max(worst, float(np.abs(g["shading_normal"][i].astype(np.float64) - want).max()))
    print(f"surface_rays {name} shading_normal: {int(k.sum())} normal-mapped hits, worst |err| = {worst:.3e} = 2^{np.log2(worst) if worst else -np.inf:.2f}")
    assert worst <= 2.0 ** -18


# ---- 9: misses, has_uv, material ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_misses_has_uv_and_material(hip, oracle, name):
    c = _case(hip, oracle, name)
    g, fs, hit = c["got"], c["fs"], c["hit"]
    miss = np.zeros(1, SURFACE_HIT_DTYPE); miss["item_index"] = 0xffffffff
    assert (_bytes(g[~hit]) == _bytes(miss)).all()
    for f in SURFACE_HIT_DTYPE.names:
        if SURFACE_HIT_DTYPE.fields[f][0].base == np.float32:
            assert np.isfinite(g[f]).all(), f
    items = g["item_index"][hit].astype(np.int64)
    assert np.array_equal(g["material"][hit], np.array([fs.items[i].material for i in items], np.int32))
    assert np.array_equal(g["has_uv"][hit], np.array([1 if any(t >= 0 for t in fs.materials[fs.items[i].material].texture) else 0 for i in items], np.uint32))
    assert (g["uv"][hit][g["has_uv"][hit] == 0] == 0.0).all()


# ---- 10: packet and tail boundaries ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_prefixes_queried_alone(hip, oracle, name):
    c = _case(hip, oracle, name)
    with hip.DeviceScene(c["fs"], 0) as ds:
        for n in (1, 63, 64, 65, 257):
            got = ds.surface_rays(c["o"][:n], c["d"][:n], 1)
            assert np.array_equal(_bytes(got), _bytes(c["got"][:n])), n
        assert len(ds.surface_rays(c["o"][:0], c["d"][:0], 1)) == 0


# ---- 11: the device form ----------------------------------------------------------------------------------------------------------
def test_device_form_equals_the_host_form(hip, oracle):
    c = _case(hip, oracle, "rich")
    L = hip.lib()
    with hip.DeviceScene(c["fs"], 0) as ds:
        to, td = torch.from_numpy(c["o"]).cuda(), torch.from_numpy(c["d"]).cuda()
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):   # the rays are produced on the stream the query runs on: no synchronisation in between
            o2, d2 = to * 1.0, td * 1.0
            res = renderer.surface_rays_torch(ds, o2, d2, 1)
        st.synchronize()
        rec = res["records"]
        assert rec.shape == (N, 32) and rec.dtype == torch.float32 and rec.is_cuda
        got = rec.cpu().numpy().view(SURFACE_HIT_DTYPE).reshape(N)
        assert np.array_equal(_bytes(got), _bytes(c["got"]))
        for f in SURFACE_HIT_DTYPE.names:   # named column views of the one tensor: no copy
            v = res[f]
            assert v.untyped_storage().data_ptr() == rec.untyped_storage().data_ptr(), f
            assert np.array_equal(_bytes(v.cpu().numpy().reshape(N, -1)), _bytes(c["got"][f].reshape(N, -1))), f
        with pytest.raises(ValueError):
            renderer.surface_rays_torch(ds, to.cpu(), td, 1)
        # refusals: nothing is launched, nothing is written
        buf = torch.full((N * 32 + 8,), SENTINEL, dtype=torch.int32, device="cuda")
        assert buf.data_ptr() % 16 == 0
        h, n = ds._h, C.c_uint32(N)
        po, pd = C.c_void_p(to.data_ptr()), C.c_void_p(td.data_ptr())
        for off in (4, 8, 12):
            assert L.rr_surface_rays_device(h, po, pd, n, 1, C.c_void_p(buf.data_ptr() + off), None) == -1
            assert b"rr_surface_rays_device" in L.rr_last_error() and b"out_dev" in L.rr_last_error()
        assert L.rr_surface_rays_device(h, C.c_void_p(to.data_ptr() + 2), pd, n, 1, C.c_void_p(buf.data_ptr()), None) == -1 and b"4-byte" in L.rr_last_error()
        host = np.zeros(N * 128 + 16, np.uint8)   # pageable host memory, 16-byte aligned
        ph = host.ctypes.data + (-host.ctypes.data) % 16
        assert L.rr_surface_rays_device(h, po, pd, n, 1, C.c_void_p(ph), None) == -1 and b"out_dev" in L.rr_last_error()
        assert L.rr_surface_rays_device(h, C.c_void_p(c["o"].ctypes.data), pd, n, 1, C.c_void_p(buf.data_ptr()), None) == -1 and b"origins_dev" in L.rr_last_error()
        assert L.rr_surface_rays_device(h, po, C.c_void_p(c["d"].ctypes.data), n, 1, C.c_void_p(buf.data_ptr()), None) == -1 and b"directions_dev" in L.rr_last_error()
        torch.cuda.synchronize()
        assert (buf.cpu().numpy().view(np.uint32) == SENTINEL).all() and not host.any()
        # and the handle answers afterwards, through the raw-pointer form on the default stream
        ds.surface_rays_device(to.data_ptr(), td.data_ptr(), N, 1, buf.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy()[:N * 32].view(np.uint8).reshape(N, 128), _bytes(c["got"]))


# ---- 12: handle state ---------------------------------------------------------------------------------------------------------------
def test_frames_around_the_query_are_unchanged(hip, oracle):
    c = _case(hip, oracle, "rich")
    cfg = make_config(samples=3, monte_carlo=True, seed=3, max_recursion=4)
    with hip.DeviceScene(c["fs"], 0) as ds:
        before = ds.render(c["cam"], cfg, aux=True)
        got = ds.surface_rays(c["o"], c["d"], 1)
        after = ds.render(c["cam"], cfg, aux=True)
    assert np.array_equal(_bytes(got), _bytes(c["got"]))
    assert_frames_identical(before, after, "rr_render around rr_surface_rays")


def test_after_scene_edits_the_query_answers_as_a_new_handle(hip, oracle):
    c = _case(hip, oracle, "rich")
    fs = c["fs"]

    def edit(drop_item):   # (a scene that has been handed to the library holds ctypes buffers and cannot be copied: build it anew)
        out = _scene("rich")
        for k, m in enumerate(out.materials):   # every value the query reports, and where it reads it from
            m.ambient_color, m.base_color, m.specular_color = tuple(m.base_color), tuple(m.specular_color), tuple(m.ambient_color)
            m.roughness, m.reflectivity, m.normal_map_strength = 0.125 + 0.01 * k, 0.25, 1.5
            m.texture = list(m.texture[1:]) + [m.texture[0]]
            m.texture_filtering_nearest = not m.texture_filtering_nearest
        if drop_item:
            del out.items[3]
        return out
    edited, fewer = edit(False), edit(True)
    with hip.DeviceScene(edited, 0) as ds:
        want_materials = ds.surface_rays(c["o"], c["d"], 1)
    with hip.DeviceScene(fewer, 0) as ds:
        want_items = ds.surface_rays(c["o"], c["d"], 1)
    with hip.DeviceScene(fs, 0) as ds:
        assert np.array_equal(_bytes(ds.surface_rays(c["o"], c["d"], 1)), _bytes(c["got"]))
        ds.update_materials(edited.materials)
        got = ds.surface_rays(c["o"], c["d"], 1)
        assert np.array_equal(_bytes(got), _bytes(want_materials))
        assert not np.array_equal(_bytes(got), _bytes(c["got"]))
        ds.set_items(fewer.items, fewer.materials)
        got = ds.surface_rays(c["o"], c["d"], 1)
        assert np.array_equal(_bytes(got), _bytes(want_items))
        assert not np.array_equal(_bytes(got), _bytes(want_materials))


def test_non_finite_rays_are_answered(hip, oracle):
    """The rays of tests/test_gpu_shade_rays.py::test_non_finite_rays_are_answered: the call returns RR_OK, and the finite rays' rows
    are unchanged."""
    c = _case(hip, oracle, "spheres_room")
    n = 64
    o, d = c["o"][:n].copy(), c["d"][:n].copy()
    o[0] = np.nan; d[1, 0] = np.inf; o[2, 1] = -np.inf; d[3] = 0.0
    with hip.DeviceScene(c["fs"], 0) as ds:
        got = ds.surface_rays(o, d, 1)
    assert np.array_equal(_bytes(got[4:]), _bytes(c["got"][4:n]))


# ---- 13: frame and queries answer from the same code ----------------------------------------------------------------------------------
def _mesh_and_ball():
    """One textured mesh (a checkered floor, bilinear) and one ball over it, under a point light (tests/corner_scenes.py's parts)."""
    from rustray_amd.flat import FlatScene, Item, Light, Material
    from tests import corner_scenes as cs
    fs = FlatScene()
    base = np.full((8, 8, 4), 255, np.uint8); base[::2, ::2, :3] = 60
    fs.textures = [base]
    fs.meshes = [cs._quad(0.0, 4.0)]
    fm = Material(base_color=(0.9, 0.8, 0.7), ambient_color=(0.1, 0.1, 0.1)); fm.texture[BASE] = 0
    cs._mesh_item(fs, 0, fm, 3, "floor")
    mi, ci = cs._mat(fs, Material(base_color=(0.2, 0.7, 0.3), ambient_color=(0.05, 0.1, 0.05)))
    t = cs.EYE.copy(); t[:3, 3] = (0.5, 1.0, -0.5); ti = cs.EYE.copy(); ti[:3, 3] = (-0.5, -1.0, 0.5)
    fs.items.append(Item(kind=0, id=6, material=mi, material_cache=ci, radius=1.0, trans=t, trans_inv=ti, bbox_min=(-1.0,) * 3, bbox_max=(1.0,) * 3, name="ball"))
    fs.lights = [Light(pos=(2.0, 7.0, 3.0), intensity=70.0)]
    cs._cam(fs, eye=(0.0, 3.0, 6.0), direction=(0.0, -0.35, -1.0))
    return fs


def test_a_frame_and_the_queries_of_its_primary_rays_agree(hip, oracle):
    """A 16 x 8 frame at 1 sample, max_recursion 0, no fog, and its 128 primary rays rebuilt on the host: the frame's kernels and the
    queries' evaluate a hit's surface, resolve a slot and seed a root record through the same functions (rr_surface.h's steps,
    rr_accumulate.h's resolve_*, root_record), so the frame IS the queries' answer -- object id and hit mask, colour bytes, and the
    depth as the accumulator holds it: round(distance * RR_DEPTH_SCALE) / RR_DEPTH_SCALE with RR_DEPTH_SCALE = 65536 (rr_device.h; one
    sample, and every distance here is far below the 512 units a 32-bit lane sum takes).  Every pixel is in every comparison."""
    from tests.helpers import as_u8
    w, h = 16, 8
    n = w * h
    fs = _mesh_and_ball()
    cam = camera_for(fs, w, h).c_struct()
    cfg = _cfg()
    table, _ = oracle.sample_table(1)
    o, d = primaries(oracle, cam, cfg, table)
    assert len(o) == n
    with hip.DeviceScene(fs, 0) as ds:
        frame = ds.render(cam, cfg, sample_xy=table, aux=True)
        surf = ds.surface_rays(o, _f32_normalised(d), 1)
        shade = ds.shade_rays(o, d, cfg, 1)
    hit = surf["hit"] == 1
    assert {3, 6} <= set(surf["object_id"][hit].tolist()) and (~hit).any()   # the mesh, the ball and the background are all in the picture
    assert np.array_equal(surf["object_id"], frame["object_id"].reshape(n))
    assert np.array_equal(hit, frame["depth"].reshape(n) > 0)
    c = np.fmin(shade["color"].astype(np.float32), np.float32(1.0)) * np.float32(255.0)   # f32::min: NaN.min(1.0) = 1.0
    assert c.dtype == np.float32 and c.shape == (n, 3)
    assert np.array_equal(as_u8(c).astype(np.uint8), frame["rgba"].reshape(n, 4)[:, :3])
    assert (frame["rgba"].reshape(n, 4)[hit, :3] != 0).any()
    x = surf["distance"] * np.float32(65536.0)
    assert x.dtype == np.float32 and float(np.abs(x).max()) < 2.0 ** 25
    want = (np.rint(x).astype(np.float64) / 65536.0).astype(np.float32)   # v_rndne: to nearest, ties to even, as numpy's rint
    assert np.array_equal(_bits(frame["depth"].reshape(n)), _bits(want))
    assert np.array_equal(_bits(shade["depth"]), _bits(want))
