"""The float64 model of uv and texture sampling (tests/uv_texture_model.py) on the CPU: hand-computed cases of the model itself, the
promise of the aimed rays of tests/uv_edge_scene.py (every case of the samplers is hit often enough, every ray hits its item), and the
oracle against the model -- the one place where the restatement and the model meet.  tests/test_gpu_uv_texture.py judges the device
with the same model.

The oracle renders frames, so its colours are those of camera rays: one camera per item (uv_edge_scene.oracle_cameras), one ray per
pixel, 1 sample, monte_carlo = 0, max_recursion = 0, no lights, and PROBE copies of the scene (uv_edge_scene.probe) in which a frame's
colour is a slot's texel.  The hit of each of those rays comes from oracle.trace_rays, its position is origin + direction * toi in
float32, and the model's uv of that position is the sampler's input.
"""
import numpy as np
import pytest

from rustray_amd.flat import make_config
from tests import uv_edge_scene as es
from tests import uv_texture_model as tm
from tests.test_gpu_shade_rays import primaries

SLOTS = (tm.BASE, tm.AMBIENT, tm.SPECULAR, tm.ALPHA, tm.ROUGHNESS, tm.AO, tm.REFLECTIVITY)

# texels written out: T22 is 2 x 2, T41 is 4 x 1, T53 is 5 wide and 3 high; texel (x, y) of T53 is (10 x + y, 100 + x, 200 + y, 50 + 10 y + x)
T22 = np.asarray([[[0, 255, 51, 102], [255, 0, 102, 51]], [[51, 102, 255, 0], [102, 51, 0, 255]]], np.uint8)
T41 = np.asarray([[[10, 20, 30, 40], [50, 60, 70, 80], [90, 100, 110, 120], [130, 140, 150, 160]]], np.uint8)
T53 = np.asarray([[[10 * x + y, 100 + x, 200 + y, 50 + 10 * y + x] for x in range(5)] for y in range(3)], np.uint8)


def _one(fn, tex, u, v):
    return fn(tex, np.float32([u]), np.float32([v]))[0]


def _texel(tex, x, y):
    return tex[y, x].astype(np.float64) / 255.0


# ---- 1: the model by hand -------------------------------------------------------------------------------------------------------------
def test_bilinear_by_hand():
    assert T22.shape == (2, 2, 4) and T41.shape == (1, 4, 4) and T53.shape == (3, 5, 4)
    # u = -0.25, width 4: x = -1 + 4 = 3.0, texel 3 exactly (floor = ceil, f = 0)
    assert np.array_equal(_one(tm.sample_bilinear, T41, -0.25, 0.0), _texel(T41, 3, 0))
    # u = 1.0: both indices clamp to the last texel, on either axis, whatever f is
    assert np.array_equal(_one(tm.sample_bilinear, T41, 1.0, 0.0), _texel(T41, 3, 0))
    assert np.array_equal(_one(tm.sample_bilinear, T53, 1.0, 1.0), _texel(T53, 4, 2))
    assert np.array_equal(_one(tm.sample_bilinear, T22, 1.0, 0.0), _texel(T22, 1, 0))
    assert np.array_equal(_one(tm.sample_bilinear, T22, 0.0, 1.0), _texel(T22, 0, 1))
    # u = -1.5, width 2: x = -3 + 2 = -1 after the ONE wrap, floor and ceil saturate to 0: texel 0
    assert np.array_equal(_one(tm.sample_bilinear, T22, -1.5, 0.0), _texel(T22, 0, 0))
    assert np.array_equal(_one(tm.sample_bilinear, T53, 0.0, -1.5), _texel(T53, 0, 0))
    # x in (width - 1, width): x0 = x1 = the last texel, exactly
    assert np.array_equal(_one(tm.sample_bilinear, T53, 0.9, 0.0), _texel(T53, 4, 0))       # x = 4.5
    assert np.array_equal(_one(tm.sample_bilinear, T53, 0.0, 0.9), _texel(T53, 0, 2))       # y = 2.7
    assert np.array_equal(_one(tm.sample_bilinear, T22, 0.75, 0.75), _texel(T22, 1, 1))
    # the interior: x = 2.5 between columns 2 and 3 (width 5), y = 1.5 between rows 1 and 2 (height 3): the mean of the four
    want = (_texel(T53, 2, 1) + _texel(T53, 3, 1) + _texel(T53, 2, 2) + _texel(T53, 3, 2)) / 4.0
    assert np.abs(_one(tm.sample_bilinear, T53, 0.5, 0.5) - want).max() < 1e-15
    # x = 0.5, y = 0.25 of the 2 x 2: 3/4 of the upper row's mean and 1/4 of the lower row's
    want = 0.75 * (_texel(T22, 0, 0) + _texel(T22, 1, 0)) / 2.0 + 0.25 * (_texel(T22, 0, 1) + _texel(T22, 1, 1)) / 2.0
    assert np.abs(_one(tm.sample_bilinear, T22, 0.25, 0.125) - want).max() < 1e-15
    # -1 <= u < 0 wraps once into the texture: u = -0.5 of width 5 is x = 2.5 as u = 0.5 is
    assert np.array_equal(_one(tm.sample_bilinear, T53, -0.5, 0.0), _one(tm.sample_bilinear, T53, 0.5, 0.0))


def test_nearest_by_hand():
    f5 = lambda x: float(np.float32(x) / np.float32(5.0))
    assert np.array_equal(_one(tm.sample_nearest, T53, f5(-0.3), 0.0), _texel(T53, 0, 0))   # -0.3 truncates toward zero
    assert np.array_equal(_one(tm.sample_nearest, T53, f5(-1.3), 0.0), _texel(T53, 4, 0))   # -1 % 5 = -1, made non-negative: 4
    assert np.array_equal(_one(tm.sample_nearest, T53, f5(6.2), 0.0), _texel(T53, 1, 0))    # periodic above 1
    assert np.array_equal(_one(tm.sample_nearest, T53, 0.0, 0.5), _texel(T53, 0, 1))        # y = 1.5 of HEIGHT 3
    assert np.array_equal(_one(tm.sample_nearest, T53, 0.5, 0.9), _texel(T53, 2, 2))
    assert np.array_equal(_one(tm.sample_nearest, T53, 1.0, 1.0), _texel(T53, 0, 0))        # u = 1 is texel 0 again: not the clamp of bilinear
    assert np.array_equal(_one(tm.sample_nearest, T22, -1.5, 0.75), _texel(T22, 1, 1))      # x = -3: -3 % 2 = -1 -> 1
    assert np.array_equal(tm.nearest_index(np.float32([np.nan, 1e30, -1e30]), 5), [0, (2 ** 31 - 1) % 5, 5 - (2 ** 31) % 5])   # saturating casts


def test_nearest_index_is_the_remainder_of_the_truncated_product():
    u = np.random.default_rng(5).uniform(-4.0, 5.0, 1000).astype(np.float32)
    for size in (8, 5):   # the mask path and the remainder path of the device
        want = [int(np.trunc(np.float32(x) * np.float32(size))) % size for x in u]
        assert np.array_equal(tm.nearest_index(u, size), want), size


def test_uv_by_hand():
    """A quad's uv under the identity, and a sphere's at its six axis points."""
    from rustray_amd.flat import Item
    fs = es.build()
    it, md = fs.items[0], fs.meshes[0]
    # A: local (x, 0, z) has u = 2.5 x and the mesh's v = -2.5 z, returned negated
    p = np.float32([[0.5, 0.0, 0.25], [-0.5, 0.0, -0.75]])
    uv, q = tm.mesh_uv64(p, it, md, np.asarray([0, 1]))
    assert np.abs(uv - [[1.25, 0.625], [-1.25, -1.875]]).max() < 1e-14
    assert np.allclose(q["A"], 4.0) and np.allclose(q["S"], 7.5)
    # face_id + n_triangles (a back face) names the same face
    assert np.array_equal(tm.mesh_uv64(p, it, md, np.asarray([2, 3]))[0], uv)
    s = Item(kind=0, id=1, material=0, material_cache=0, radius=2.0)
    p = np.float32([[2, 0, 0], [0, 0, -2], [-2, 0, 1e-30], [0, 0, 2], [0.02, -2, 0], [0.02, 2, 0]])
    uv, q = tm.sphere_uv64(p, s)
    assert np.abs(uv[:4, 0] - [0.5, 0.75, 0.0, 0.25]).max() < 1e-15 and np.abs(uv[:4, 1] + 0.5).max() < 1e-15
    assert abs(uv[4, 1]) < 1e-15 and abs(uv[5, 1] + 1.0) < 1e-15      # -y / r = 1: v = 0;  -y / r = -1: v = -1


# ---- 2: the aimed rays keep their promise ---------------------------------------------------------------------------------------------
_cache = {}


def _aimed(oracle):
    if "aimed" not in _cache:
        c = es.rays()
        fs = c["fs"]
        found, item, face, toi = oracle.trace_rays(fs.c_struct(), c["o"], c["d"], 1)
        c.update(found=found, hit_item=item, face=face, position=es.f32_position(c["o"], c["d"], toi))
        c["uv"], c["tol"], c["sphere"], c["omt2"] = es.model_uv(fs, c["item"], face, c["position"])
        _cache["aimed"] = c
    return _cache["aimed"]


def test_every_ray_hits_the_item_it_is_aimed_at(oracle):
    c = _aimed(oracle)
    assert 1500 <= len(c["o"]) <= 2500
    assert c["found"].all() and np.array_equal(c["hit_item"], c["item"])
    assert np.array_equal(np.sort(c["interleaved"]), np.arange(len(c["o"])))
    mesh = ~c["sphere"]
    assert (c["face"][mesh] < 16).all()   # front faces
    assert c["omt2"].min() >= 2.0 ** -16
    grid, seam, polar = (c["kind"] == k for k in (0, 1, 2))
    assert (c["omt2"][c["sphere"] & grid] >= 2.0 ** -8).all()
    assert int(seam.sum()) == 64 and int(polar.sum()) == 64
    assert ((c["omt2"][polar] >= 2.0 ** -16) & (c["omt2"][polar] < 2.0 ** -8)).all()
    theta = c["uv"][seam, 0] * 2.0 * np.pi - np.pi
    assert (np.pi - np.abs(theta) < 2.0 ** -6).all() and (theta > 0).sum() >= 16 and (theta < 0).sum() >= 16


def test_every_regime_is_hit(oracle):
    c = _aimed(oracle)
    es.assert_regimes(es.regime_counts(c["fs"], c["item"], c["uv"]), "aimed rays, model uv")


def test_item_d_pins_its_uv(oracle):
    """A constant uv c comes back as c (a1 + a2 + a3): within 8 ulp of c."""
    c = _aimed(oracle)
    for it in (3, 4):
        s = np.flatnonzero(c["item"] == it)
        for i in s:
            u, v = es.d_cell_uv(8 * (it - 3) + int(c["face"][i]) // 2)
            assert abs(c["uv"][i, 0] - float(u)) <= 8 * tm.U * abs(float(u)) and abs(c["uv"][i, 1] - float(v)) <= 8 * tm.U * abs(float(v))


# ---- 3: the oracle against the model --------------------------------------------------------------------------------------------------
def _cfg():
    return make_config(samples=1, monte_carlo=False, seed=3, max_recursion=0, fog_density=0.0)


def _frames(oracle, group):
    """The camera rays of a group's frame, their hits and model uv, and the oracle's mean_rgb per slot that an item of the group maps."""
    if group not in _cache:
        fs = es.build()
        probes = {s: es.probe(fs, s) for s in SLOTS}
        cam = es.oracle_cameras(fs)[group]
        cfg = _cfg()
        table, _ = oracle.sample_table(1)
        o, d = primaries(oracle, cam, cfg, table)
        d = es.f32_normalised(d)
        found, item, face, toi = oracle.trace_rays(fs.c_struct(), o, d, 1)
        want = [k for k, g in enumerate(es.ITEM_GROUP) if es.GROUPS[g] == group]
        keep = found & np.isin(item, want)
        pos = es.f32_position(o, d, toi)
        c = dict(fs=fs, keep=keep, item=item, face=face)
        c["uv"], c["tol"], c["sphere"], c["omt2"] = es.model_uv(fs, np.where(keep, item, -1), face, pos)
        slots = [s for s in SLOTS if any(es.material_of(fs, k).texture[s] >= 0 for k in want)]
        c["rgb"] = {s: oracle.render(probes[s].c_struct(), cam, cfg, sample_xy=table, want_means=True, n_threads=8)["mean_rgb"].reshape(-1, 3) for s in slots}
        _cache[group] = c
    return _cache[group]


def test_oracle_samples_item_d_as_the_model(oracle):
    """Item D's bilinear cells away from a boundary: |oracle - model| <= 2^-21 + 2^-20 max(width, height), a uv error of 2^-20 times
    the largest possible texel slope, which is the size."""
    c = _frames(oracle, "D")
    fs = c["fs"]
    m = es.material_of(fs, 3)
    combos, worst = 0, 0.0
    for slot in (tm.BASE, tm.AMBIENT):
        tex = fs.textures[m.texture[slot]]
        h, w = tex.shape[:2]
        for cell in range(8):
            u, v = es.d_cell_uv(cell)
            x, y = float(u) * w, float(v) * h
            if abs(x - round(x)) < 0.25 or abs(y - round(y)) < 0.25:
                continue   # (left to the GPU test, where the device's own uv is the input)
            s = c["keep"] & (c["item"] == 3) & (c["face"] // 2 == cell)
            assert int(s.sum()) >= 16, (slot, cell, int(s.sum()))
            want = tm.sample_bilinear(tex, c["uv"][s, 0].astype(np.float32), c["uv"][s, 1].astype(np.float32))[:, :3]
            err = np.abs(c["rgb"][slot][s] - want).max()
            bound = 2.0 ** -21 + 2.0 ** -20 * max(w, h)
            worst = max(worst, err / bound)
            assert err <= bound, (slot, cell, err, bound)
            combos += 1
    print(f"oracle against model, item D: {combos} (cell, slot) pairs, worst |err| / bound = {worst:.4f}")
    assert combos >= 2


@pytest.mark.parametrize("group", ("A", "B", "C", "E", "F"))
def test_oracle_colours_are_the_models(oracle, group):
    """Every slot the item maps, at the model's uv: |oracle - model| <= 2^-21 + max(tol_u, tol_v) max(width, height) with the uv bounds
    of the GPU test, on the hits whose float64 position is at least 2^-12 from every whole number (0 included) on both axes -- at
    least 90 % of the item's hits."""
    c = _frames(oracle, group)
    fs = c["fs"]
    k = [i for i, g in enumerate(es.ITEM_GROUP) if es.GROUPS[g] == group][0]
    m = es.material_of(fs, k)
    hits = c["keep"] & (c["omt2"] >= 2.0 ** -16)
    assert int(hits.sum()) >= 100, int(hits.sum())
    uv32 = c["uv"].astype(np.float32)
    for slot, rgb in c["rgb"].items():
        tex = fs.textures[m.texture[slot]]
        h, w = tex.shape[:2]
        x, y = c["uv"][:, 0] * w, c["uv"][:, 1] * h
        s = hits & (np.abs(x - np.rint(x)) >= 2.0 ** -12) & (np.abs(y - np.rint(y)) >= 2.0 ** -12)
        share = s.sum() / hits.sum()
        want = tm.sample(m, fs.textures, slot, uv32[s, 0], uv32[s, 1])[:, :3]
        bound = 2.0 ** -21 + c["tol"][s].max(axis=1) * max(w, h)
        err = np.abs(rgb[s] - want).max(axis=1)
        print(f"oracle against model, item {group} slot {slot} ({w} x {h}): {int(s.sum())} of {int(hits.sum())} hits ({share:.3f}), worst |err| / bound = {(err / bound).max():.4f}")
        assert share >= 0.9, (group, slot, share)
        assert (err <= bound).all(), (group, slot, float((err / bound).max()))
