"""The device's uv and every value it samples from a texture, against the float64 model of tests/uv_texture_model.py -- written from
the reference's text, not from the device code or the oracle -- on the scene and the aimed rays of tests/uv_edge_scene.py: about 1 700
rays in one rr_surface_rays call per ray order, and two 16 x 8 frames through rr_render_pixels.  tests/test_uv_texture_model_host.py
holds the model's own hand-computed cases and the oracle to the same model on the CPU.

uv is judged at the device's own f32 `position` and `face_id`; the sampled values at the device's own f32 `uv`, so a texel boundary a
few ulp away is the same boundary for both sides.  Nothing is left out of any comparison.

One MI355X, worst |err| / bound:

    mesh uv (992 hits): A 0.0938, B 0.0516, C 0.1130, D 0.0213
    sphere uv (704 hits): grid 0.1169 (u) 0.0814 (v), seam 0.0672 / 0.0583, poles 0.0508 / 0.0475
    sampled values, bilinear materials, all seven slots: 0.2615; nearest-filter materials: every word bit-equal
    interleaved against grouped ray order: byte-equal records
    frames: |colour - ambient_color| at most 2^-25 = 0.0312 BAND_EPS_ABS in both; |colour - model| 0.0685 (one item) and 0.0439
    (two items) of BAND_EPS_ABS + 2^-21
    regimes on the device's uv, fewest hits: 24 (a boundary approached from above), 30 (only the second index clamped, v)
"""
import numpy as np
import pytest

from rustray_amd.flat import make_config
from tests import uv_edge_scene as es
from tests import uv_texture_model as tm
from tests.helpers import BAND_EPS_ABS
from tests.test_gpu_shade_rays import primaries

pytestmark = pytest.mark.gpu

_cache = {}
LUT = (np.arange(256, dtype=np.float32) / np.float32(255.0)).astype(np.float32)   # (p as f32) / 255.0


def _bytes(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(len(a), -1)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _case(hip, oracle):
    if not _cache:
        c = es.rays()
        fs = c["fs"]
        cfg = make_config(samples=1, monte_carlo=False, seed=3, max_recursion=0, fog_density=0.0)
        table, _ = oracle.sample_table(1)
        perm = c["interleaved"]
        frames = []
        with hip.DeviceScene(fs, 0) as ds:
            c["got"] = ds.surface_rays(c["o"], c["d"], 1)
            c["got_interleaved"] = ds.surface_rays(np.ascontiguousarray(c["o"][perm]), np.ascontiguousarray(c["d"][perm]), 1)
            for cam in es.frame_cameras():
                o, d = primaries(oracle, cam, cfg, table)
                frames.append(dict(pixels=ds.render_pixels(cam, cfg, sample_xy=table), surf=ds.surface_rays(o, es.f32_normalised(d), 1), w=cam.width, h=cam.height))
        c["frames"] = frames
        g = c["got"]
        g.setflags(write=False)
        assert (g["hit"] == 1).all() and np.array_equal(g["item_index"], c["item"]), "a ray missed the item it was aimed at"
        assert (g["has_uv"] == 1).all()
        c["uv64"], c["tol"], c["sphere"], c["omt2"] = es.model_uv(fs, g["item_index"], g["face_id"], g["position"])
        _cache.update(c)
    return _cache


def _ratio(err, bound):
    """err / bound, with 0 / 0 = 0 (a bound of zero asks for equality)."""
    return np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))


# ---- uv -------------------------------------------------------------------------------------------------------------------------------
def test_mesh_uv_against_float64(hip, oracle):
    """Items A, B, C, D, every hit: |uv_dev - mesh_uv64| <= 4 * 2^-24 * S * (L^2 / A + P L / A + 1) per component
    (uv_texture_model.mesh_uv_bound has the count)."""
    c = _case(hip, oracle)
    s = ~c["sphere"]
    assert int(s.sum()) == 3 * 288 + 128
    err = np.abs(c["got"]["uv"][s].astype(np.float64) - c["uv64"][s])
    r = _ratio(err, c["tol"][s])
    for k in range(5):
        print(f"mesh uv, item {c['fs'].items[k].name}: worst |err| / bound = {r[c['item'][s] == k].max():.4f}")
    assert np.isfinite(c["got"]["uv"][s]).all() and (err <= c["tol"][s]).all(), float(r.max())


def test_sphere_uv_against_float64(hip, oracle):
    """Items E and F, every hit: u on the circle within tol_u, v within tol_v (uv_texture_model.sphere_uv_bounds)."""
    c = _case(hip, oracle)
    s = c["sphere"]
    assert int(s.sum()) == 2 * (288 + 64) and c["omt2"][s].min() >= 2.0 ** -16
    uv = c["got"]["uv"][s].astype(np.float64)
    assert np.isfinite(uv).all()
    eu = tm.circle_distance(uv[:, 0], c["uv64"][s, 0])
    ev = np.abs(uv[:, 1] - c["uv64"][s, 1])
    ru, rv = eu / c["tol"][s, 0], ev / c["tol"][s, 1]
    for kind, name in enumerate(("grid", "seam", "poles")):
        k = c["kind"][s] == kind
        print(f"sphere uv, {name}: worst |err| / bound = {ru[k].max():.4f} (u), {rv[k].max():.4f} (v)")
    assert (ru <= 1.0).all() and (rv <= 1.0).all(), (float(ru.max()), float(rv.max()))
    # the seam is met from both sides: u near 0 and u near 1
    seam = uv[c["kind"][s] == 1, 0]
    assert (seam < 0.01).sum() >= 16 and (seam > 0.99).sum() >= 16


# ---- sampled values -------------------------------------------------------------------------------------------------------------------
def _check_values(fs, rec, what):
    """Every colour and scalar map of the hit records `rec` against the model at the records' own uv.  Nearest-filter materials: the bits
    of f32(material colour) * f32(i / 255).  Bilinear: |got - model| <= 2^-21 |material factor| -- three interpolation levels of three
    roundings each on values in [0, 1], then the product; where a coordinate is clamped or saturated both texels of that axis are one
    texel and f multiplies an exact zero -- and 2^-20 |factor| for alpha and roughness, which take one more product each.  Returns
    the worst |err| / bound of the bilinear hits."""
    worst = 0.0
    for k in np.unique(rec["item_index"]):
        s = rec["item_index"] == k
        m = es.material_of(fs, k)
        g = rec[s]
        u, v = np.ascontiguousarray(g["uv"][:, 0]), np.ascontiguousarray(g["uv"][:, 1])
        model = tm.surface_model(m, fs.textures, u, v)
        n = len(g)
        rgb1 = {f: np.asarray(list(getattr(m, f)) + [1.0], np.float32) for f in ("base_color", "ambient_color", "specular_color")}
        if m.texture_filtering_nearest:
            assert all(m.texture[t] < 0 for t in (tm.ALPHA, tm.ROUGHNESS, tm.AO, tm.REFLECTIVITY))
            for f, slot in (("base_color", tm.BASE), ("ambient_color", tm.AMBIENT), ("specular_color", tm.SPECULAR)):
                want = np.tile(rgb1[f], (n, 1))
                if m.texture[slot] >= 0:
                    tex = fs.textures[m.texture[slot]]
                    want = want * LUT[tex[tm.nearest_index(v, tex.shape[0]), tm.nearest_index(u, tex.shape[1])]]
                assert want.dtype == np.float32
                width = g[f].shape[1]
                assert np.array_equal(_bits(g[f]), _bits(want[:, :width])), (what, fs.items[k].name, f)
            alpha = np.float32(m.alpha) * g["base_color"][:, 3]
            assert alpha.dtype == np.float32 and np.array_equal(_bits(g["alpha"]), _bits(alpha))
            assert (g["roughness"] == np.float32(m.roughness)).all() and (g["reflectivity"] == np.float32(m.reflectivity)).all() and (g["ambient_occlusion"] == 1.0).all()
            continue
        for f in ("base_color", "ambient_color", "specular_color"):
            width = g[f].shape[1]
            bound = 2.0 ** -21 * np.abs(rgb1[f][:width].astype(np.float64))
            err = np.abs(g[f].astype(np.float64) - model[f])
            worst = max(worst, float(_ratio(err, np.broadcast_to(bound, err.shape)).max()))
            assert (err <= bound).all(), (what, fs.items[k].name, f, float(_ratio(err, np.broadcast_to(bound, err.shape)).max()))
        for f, bound in (("ambient_occlusion", 2.0 ** -21), ("reflectivity", 2.0 ** -21), ("alpha", 2.0 ** -20 * abs(float(np.float32(m.alpha)))),
                         ("roughness", 2.0 ** -20 / (2.0 * np.pi))):
            err = np.abs(g[f].astype(np.float64) - model[f])
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (what, fs.items[k].name, f, float((err / bound).max()))
    return worst


def test_every_sampled_value_against_the_model(hip, oracle):
    c = _case(hip, oracle)
    worst = _check_values(c["fs"], c["got"], "aimed rays")
    print(f"sampled values, bilinear: worst |err| / bound = {worst:.4f}")
    es.assert_regimes(es.regime_counts(c["fs"], c["got"]["item_index"], c["got"]["uv"].astype(np.float64)), "aimed rays, device uv")


def test_ray_order_does_not_change_an_answer(hip, oracle):
    """Interleaved, every wave holds all seven items; grouped, most waves hold one."""
    c = _case(hip, oracle)
    perm = c["interleaved"]
    assert not np.array_equal(perm, np.arange(len(perm)))
    assert np.array_equal(_bytes(c["got_interleaved"]), _bytes(c["got"][perm]))


# ---- the frame's own kernels ----------------------------------------------------------------------------------------------------------
def test_level_one_frames_sample_as_the_query(hip, oracle):
    """1 sample, monte_carlo = 0, max_recursion = 0, no fog, no lights: a pixel's colour is its hit's ambient colour.  Frame 1 lies inside
    item A -- waves of one item, which read material and texture descriptor on the scalar path --, frame 2 across the border of A and
    B.  Per pixel: the colour within BAND_EPS_ABS of rr_surface_rays' ambient_color for the same ray (the accumulator's fixed point),
    and within BAND_EPS_ABS + 2^-21 of the model at that record's uv."""
    c = _case(hip, oracle)
    fs = c["fs"]
    for number, fr in enumerate(c["frames"], 1):
        surf, px = fr["surf"], fr["pixels"]
        n = fr["w"] * fr["h"]
        assert len(surf) == n == 128 and (surf["hit"] == 1).all()
        assert np.array_equal(px["object_id"], surf["object_id"])
        ids = surf["object_id"].reshape(fr["h"], fr["w"])
        if number == 1:
            assert (ids == fs.items[0].id).all()
        else:
            assert set(np.unique(ids)) == {fs.items[0].id, fs.items[1].id}
            assert sum(len(np.unique(row)) == 2 for row in ids) >= 6
        colour = px["color"].astype(np.float64)
        assert np.isfinite(colour).all()
        e1 = np.abs(colour - surf["ambient_color"].astype(np.float64)).max()
        print(f"frame {number}: worst |colour - ambient_color| = {e1:.3e} = {e1 / BAND_EPS_ABS:.4f} BAND_EPS_ABS")
        assert e1 <= BAND_EPS_ABS
        worst = _check_values(fs, surf, f"frame {number}")
        model = np.zeros((n, 3))
        for k in np.unique(surf["item_index"]):
            s = surf["item_index"] == k
            model[s] = tm.surface_model(es.material_of(fs, k), fs.textures, np.ascontiguousarray(surf["uv"][s, 0]), np.ascontiguousarray(surf["uv"][s, 1]))["ambient_color"]
        e2 = np.abs(colour - model).max()
        print(f"frame {number}: worst |colour - model| = {e2:.3e} = {e2 / (BAND_EPS_ABS + 2.0 ** -21):.4f} of the bound; records against the model: {worst:.4f}")
        assert e2 <= BAND_EPS_ABS + 2.0 ** -21
