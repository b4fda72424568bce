"""The receiver of a level-1 packet through the scalar cache.  With sample_group 64 a level-1 packet is the 64 samples of one pixel:
as a rule all of its hits lie on ONE item, and k_shade<true> then fetches that item's words, its material and the texture
descriptors once per wave (rr_surface.h load_hit_item_uniform, load_material_uniform, tex_color) where packets of several items
load per lane.  Nothing may change by a bit.  The tail of k_trace_shadow<true> reads the same receiver after the walk (its material's
alpha, the occluder's alpha texture at the receiver's uv); the forms of it that were tried on the scalar path are not shipped
(profiles/r14_dropped.txt), and test_shadow_tail holds whatever form it takes to the oracle.

The levers: rr_tuning::sample_group (64: uniform packets; 4 and 1: packets of 16 and 64 pixels, mixed at every item edge and at
the horizon) and tests/packet_pad.py (7 items: level 1 on the dense shadow queue, the loader in front of wave_alloc; 17 and 65:
packet form, fixed shadow slots, side-by-side stages).  Frames are 32 x 16 at 64 samples with monte_carlo."""
import copy

import numpy as np
import pytest

from rustray_amd.flat import FlatScene, Item, Light, Material, MeshData, make_config
from rustray_amd.scene import get_transformation, inverse_affine
from tests.corner_scenes import _quad
from tests.helpers import assert_frames_identical, camera_for, compare_frames
from tests.packet_pad import in_packet_range, pad_inert
from tests.test_gpu_packet_walk import _add, _ball, _camera, lights_scene
from tests.test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu
COUNTS = ("primary_rays", "secondary_rays", "shaded_hits", "shadow_rays")
W, H = 32, 16
GROUPS = (64, 4, 1)


def _cfg():
    return make_config(samples=64, monte_carlo=True, seed=5, max_recursion=3)


def _clone(fs):
    return pad_inert(fs, len(fs.items), "copies")


def _frame(ds, fs):
    out = ds.render(camera_for(fs, W, H).c_struct(), _cfg())
    st = ds.stats()
    return out, [st[k] for k in COUNTS]


def _render(hip, fs, group=64, compat=0):
    with hip.DeviceScene(fs, 0) as ds:
        ds.set_tuning(sample_group=group)
        if compat:
            ds.set_compat(compat)
        return _frame(ds, fs)


def _same(a, b, what):
    assert_frames_identical(a[0], b[0], what)
    assert a[1] == b[1], (what, a[1], b[1])


# ---------------------------------------------------------------------------------------------------------------------------
# sample groups and scene sizes
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lights_reference(hip):
    """lights_scene unpadded (7 items) at sample_group 64: computed once."""
    fs = lights_scene()
    assert not in_packet_range(len(fs.items))
    out, counts = _render(hip, fs)
    ids = out["object_id"]
    assert (ids == 0).any() and counts[3] > 0                          # part of the frame sees no item
    blocks = ids.reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 64)
    n_kinds = [len(np.unique(b)) for b in blocks]
    assert sum(k > 1 for k in n_kinds) >= 5                            # item boundaries cross most 8 x 8 blocks
    assert any((b == 0).any() and (b != 0).any() for b in blocks)      # blocks with missing and hitting pixels
    assert any((b == 0).all() for b in ids.reshape(-1, 16))            # runs of 16 pixels that all miss
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out, counts


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("n", (7, 17, 65))
def test_sample_groups_and_scene_sizes_give_one_frame(hip, lights_reference, n, group):
    """sample_group 64 (one pixel per packet: the uniform loader), 4 and 1 (16 and 64 pixels per packet: mixed) on the scene at 7 items
    (dense shadow queue), 17 and 65 (packet form, fixed slots): all four buffers and the four ray counts are those of the reference."""
    fs = lights_scene()
    if n != len(fs.items):
        fs = pad_inert(fs, n, "scattered", seed=n)
    assert in_packet_range(len(fs.items)) == (n >= 17)
    _same(_render(hip, fs, group), lights_reference, f"{n} items, sample_group {group}")


# ---------------------------------------------------------------------------------------------------------------------------
# a materials scene against the oracle
# ---------------------------------------------------------------------------------------------------------------------------
def _grid_mesh(seed):
    """A 3 x 3 height field with per-vertex normals and uvs (eight triangles)."""
    rng = np.random.default_rng(seed)
    xs, zs = np.meshgrid(np.linspace(-1.0, 1.0, 3), np.linspace(-1.0, 1.0, 3), indexing="ij")
    p = np.stack([xs.ravel(), rng.uniform(0.0, 0.5, 9), zs.ravel()], axis=1).astype(np.float32)
    nrm = np.stack([rng.uniform(-0.4, 0.4, 9), np.ones(9), rng.uniform(-0.4, 0.4, 9)], axis=1)
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    uv = np.stack([(xs.ravel() + 1.0) * 0.7, (zs.ravel() + 1.0) * 0.6], axis=1).astype(np.float32)   # beyond 1: the wrap
    tri = []
    for i in range(2):
        for j in range(2):
            a, b, c, d = 3 * i + j, 3 * (i + 1) + j, 3 * (i + 1) + j + 1, 3 * i + j + 1
            tri += [[a, d, c], [a, c, b]]
    tri = np.asarray(tri, np.uint32)
    return MeshData(positions=p, indices=tri, uvs=uv, uv_indices=tri.copy(), normals=nrm, normal_indices=tri.copy())


def _mesh_item(fs, mesh, idn, centre, rot, m, name, flip=False):
    fs.meshes.append(mesh)
    t = get_transformation(np.eye(4, dtype=np.float32), centre, (1.0, 1.0, 1.0), rot)
    lo, hi = mesh.positions.min(0), mesh.positions.max(0)
    _add(fs, Item(kind=1, id=idn, material=0, material_cache=0, mesh=len(fs.meshes) - 1, trans=t, trans_inv=inverse_affine(t),
                  bbox_min=tuple(float(v) for v in lo), bbox_max=tuple(float(v) for v in hi), flip_normals=flip, name=name), m)


def materials_scene():
    """Eight items: every texture slot under both filters, a texture whose size is no power of two, smooth / flat / flipped meshes, a
    textured sphere, alpha < 1, reflectivity, roughness, receive_shadow off, monte_carlo off, an alpha-mapped occluder over opaque
    and translucent receivers, three lights with a disabled one between two enabled ones."""
    fs = FlatScene()
    rng = np.random.default_rng(23)

    def image(h, w, lo=40):
        t = rng.integers(lo, 256, (h, w, 4)).astype(np.uint8); t[..., 3] = 255
        return t
    mask = np.zeros((8, 8, 4), np.uint8); mask[..., :3] = (rng.integers(0, 2, (8, 8, 1)) * 255).astype(np.uint8); mask[..., 3] = 255
    fs.textures = [image(8, 8), image(3, 5), image(4, 4), image(8, 4), mask, image(4, 8, 0), image(2, 2, 128), image(4, 4, 0), image(6, 7)]
    #               0 base     1 (5 x 3)    2            3 normal     4 alpha 5 roughness    6 ao             7 reflectivity  8 (7 x 6)
    floor = Material(base_color=(0.8, 0.8, 0.8)); floor.texture[0] = 1                       # bilinear, 5 x 3
    fs.meshes.append(_quad(0.0, 12.0))
    eye = np.eye(4, dtype=np.float32)
    _add(fs, Item(kind=1, id=2, material=0, material_cache=0, mesh=0, trans=eye.copy(), trans_inv=eye.copy(),
                  bbox_min=(-12.0, 0.0, -12.0), bbox_max=(12.0, 0.0, 12.0), name="floor"), floor)
    glass = Material(base_color=(0.5, 0.8, 0.9), alpha=0.4, refraction_index=1.2)            # a translucent RECEIVER under the balls
    _mesh_item(fs, _quad(0.0, 2.5), 3, (-2.5, 0.05, -3.0), (0.0, 0.0, 0.0), glass, "glass")
    every = Material(base_color=(0.9, 0.9, 0.9), ambient_color=(0.1, 0.1, 0.1), texture_filtering_nearest=True, roughness=0.05)
    every.texture = [0, 8, 2, 3, 4, 5, 6, 7]                                                 # all eight slots, nearest, one 7 x 6
    _ball(fs, 10, (-1.0, 0.95, -3.0), 0.8, every)
    _ball(fs, 11, (2.5, 0.8, -5.0), 0.7, Material(base_color=(0.4, 0.5, 0.7), reflectivity=0.5, roughness=0.1, shininess=40.0))
    smooth = Material(base_color=(0.9, 0.8, 0.7), ambient_color=(0.05, 0.05, 0.05))
    smooth.texture = [8, 0, 2, 3, 4, 5, 6, 7]                                                # all eight slots, bilinear
    _mesh_item(fs, _grid_mesh(1), 20, (0.8, 0.3, -1.2), (0.2, 0.4, 0.0), smooth, "smooth")
    flat = Material(base_color=(0.3, 0.9, 0.4), smooth_shading=False, receive_shadow=False)
    _mesh_item(fs, _grid_mesh(2), 21, (3.2, 0.4, -2.0), (0.0, 0.3, 0.2), flat, "flat_flipped", flip=True)
    matte = Material(base_color=(0.9, 0.3, 0.3), monte_carlo=False, roughness=0.2, shadow_softness=0.05)
    _mesh_item(fs, _grid_mesh(3), 22, (-3.6, 0.6, -6.0), (0.5, 0.0, 0.1), matte, "no_monte_carlo")
    cover = Material(base_color=(0.9, 0.4, 0.2)); cover.texture[4] = 4                       # an occluder with an alpha texture
    _mesh_item(fs, _quad(0.0, 1.6), 30, (-1.0, 2.4, -3.5), (0.3, 0.0, 0.2), cover, "alpha_cover")
    fs.lights = [Light(pos=(-0.5, 5.0, -2.0), intensity=120.0),
                 Light(pos=(3.0, 4.0, 0.0), intensity=80.0, enabled=False),
                 Light(dir=(0.4, -1.0, -0.3), intensity=0.5, light_type=0, color=(1.0, 0.9, 0.8))]
    _camera(fs, (0.0, 3.0, 5.0), (0.0, -0.3, -1.0))
    return fs


@pytest.fixture(scope="module")
def materials(hip, oracle):
    """The scene, the oracle's frame with its float64 means, and the device frames by (items, sample_group, compat): each computed once."""
    fs = materials_scene()
    assert not in_packet_range(len(fs.items))
    cam = camera_for(fs, W, H).c_struct()
    ref = oracle.render(fs.c_struct(), cam, _cfg(), want_means=True, n_threads=16)
    forms = {len(fs.items): fs, 17: pad_inert(fs, 17, "switches", seed=17)}
    cache = {}

    def frame(n, group=64, compat=0):
        if (n, group, compat) not in cache:
            cache[n, group, compat] = _render(hip, forms[n], group, compat)
        return cache[n, group, compat]
    return fs, ref, frame


def test_materials_scene_matches_the_oracle(materials):
    """Unpadded (dense queue) and padded to 17 with the switch items (packet form, and the projective inverse: general_w), sample_group 64."""
    fs, ref, frame = materials
    ids = np.unique(ref["object_id"]).tolist()
    assert all(i in ids for i in (0, 2, 3, 10, 11, 20, 21, 22, 30)), ids
    for n in (len(fs.items), 17):
        assert_parity(frame(n)[0], ref, f"{n} items")
    _same(frame(17), frame(len(fs.items)), "17 items against unpadded")


def test_shadow_tail(materials, oracle):
    """Opaque and alpha 0.4 receivers under an alpha-mapped occluder and opaque balls: sample_group 64 (one receiver per shadow packet) and 1
    (receivers of several items in one packet), 8 items (dense queue) and 17 (fixed slots), against the oracle and each other; then the
    occluder-alpha compatibility switch, which takes the occluder's material instead."""
    fs, ref, frame = materials
    n0 = len(fs.items)
    for group in (64, 1):
        assert_parity(frame(17, group)[0], ref, f"17 items, sample_group {group}")
        _same(frame(n0, group), frame(17, group), f"sample_group {group}: 8 items against 17")
    _same(frame(17, 1), frame(17, 64), "sample_group 1 against 64")
    assert frame(17)[1][3] > 0
    oracle.lib().rro_set_shot_era(1)
    try:
        era = oracle.render(fs.c_struct(), camera_for(fs, W, H).c_struct(), _cfg(), n_threads=16)
    finally:
        oracle.lib().rro_set_shot_era(0)
    assert not np.array_equal(era["rgba"], ref["rgba"])                 # the factor 1 - alpha matters in this frame
    for group in (64, 1):
        res = compare_frames(frame(17, group, 1)[0], era)
        assert res["n_rgb_over"] == 0 and res["n_id_diff"] == 0, (group, res)
        _same(frame(n0, group, 1), frame(17, group, 1), f"compat, sample_group {group}: 8 items against 17")


# ---------------------------------------------------------------------------------------------------------------------------
# live edits
# ---------------------------------------------------------------------------------------------------------------------------
def test_frames_after_edits_equal_fresh_scenes(hip):
    """One handle in packet range; between frames a material, a texture, a light and an item's visibility are edited.  After each the
    frame and the ray counts equal those of a scene created in that state: the receiver's records are read again in every launch."""
    p = pad_inert(materials_scene(), 20, "scattered", seed=20)
    assert in_packet_range(len(p.items))
    recoloured = _clone(p)
    for idx in (recoloured.items[0].material, recoloured.items[0].material_cache):
        recoloured.materials[idx].base_color = (0.3, 0.5, 0.9)
    for idx in (recoloured.items[3].material, recoloured.items[3].material_cache):
        recoloured.materials[idx].alpha = 0.6
    retextured = _clone(recoloured)
    rng = np.random.default_rng(31)
    img = rng.integers(0, 256, (5, 6, 4)).astype(np.uint8); img[..., 3] = 255
    retextured.textures.append(img)
    retextured.materials[retextured.items[0].material].texture[0] = len(retextured.textures) - 1
    relit = _clone(retextured)
    relit.lights = copy.deepcopy(relit.lights)
    relit.lights[0].pos = (1.5, 4.0, -1.0)
    relit.lights[1].enabled = True
    hidden = _clone(relit)
    hidden.items[2].visible = False                                      # the textured ball
    states = [("created", p), ("material", recoloured), ("texture", retextured), ("light", relit), ("visibility", hidden)]
    fresh = {what: _render(hip, _clone(fs)) for what, fs in states}
    frames = [fresh[what][0] for what, _ in states]
    for a, b in zip(frames, frames[1:]):                                 # every edit changes the picture: a stale record could not pass
        assert any(not np.array_equal(a[k], b[k]) for k in ("rgba", "depth", "object_id"))
    with hip.DeviceScene(p, 0) as ds:
        for what, fs in states:
            if what == "material":
                ds.update_materials(fs.materials)
            elif what == "texture":
                assert ds.add_textures([img]) == len(fs.textures) - 1
                ds.update_materials(fs.materials)
            elif what == "light":
                ds.update_lights(fs.lights)
            elif what == "visibility":
                ds.update_item_flags([it.visible for it in fs.items], [it.flip_normals for it in fs.items])
            _same(_frame(ds, fs), fresh[what], what)
