"""Scene life cycle through the C ABI on the GPU: degenerate scenes (empty meshes, no items), repeated create / destroy
without leaking HBM, material edits between frames (rr_scene_update_materials vs a freshly created scene), and updates that
are refused or fail part-way: they leave the scene rendering exactly what it rendered before."""
import copy
import ctypes as C

import numpy as np
import pytest

from rustray_amd.flat import Item, MeshData, make_config
from tests.helpers import assert_frames_identical, assert_in_band, camera_for, compare_frames, item_transforms, load_scene, with_transforms

pytestmark = pytest.mark.gpu


def _same(a, b):
    for k in ("rgba", "depth", "object_id"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["normal"], b["normal"], equal_nan=True)


def test_empty_mesh_item_is_legal_and_invisible(hip, oracle):
    """A mesh without faces (an OBJ group or glTF primitive with no triangles) used to crash the host-side BVH collapse."""
    fs = load_scene("spheres")
    base = copy.deepcopy(fs)
    fs.meshes.append(MeshData(positions=np.zeros((0, 3), np.float32), indices=np.zeros((0, 3), np.uint32)))
    it = copy.deepcopy(fs.items[0])
    it.kind, it.mesh, it.id, it.name = 1, len(fs.meshes) - 1, 999, "empty"
    it.bbox_min, it.bbox_max = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
    fs.items.append(it)
    cam = camera_for(fs, 96, 96).c_struct()
    cfg = make_config(samples=2, monte_carlo=True, seed=4)
    with hip.DeviceScene(fs, 0) as ds, hip.DeviceScene(base, 0) as ds0:
        out, ref = ds.render(cam, cfg), ds0.render(cam, cfg)
        _same(out, ref)
    res = compare_frames(out, oracle.render(fs.c_struct(), cam, cfg, want_means=True, n_threads=4))
    assert res["n_rgb_over"] == 0 and res["n_id_diff"] == 0, res
    assert_in_band(res)


def test_scene_without_items_renders_black_and_accepts_updates(hip):
    fs = load_scene("spheres")
    fs.items = []
    cam = camera_for(fs, 64, 48).c_struct()
    cfg = make_config(samples=2, monte_carlo=True, seed=1)
    with hip.DeviceScene(fs, 0) as ds:
        ds.update_transforms(np.zeros((0, 4, 4), np.float32), np.zeros((0, 4, 4), np.float32))
        out = ds.render(cam, cfg)
        st = ds.stats()
    assert (out["rgba"][..., :3] == 0).all() and (out["rgba"][..., 3] == 255).all() and (out["object_id"] == 0).all()
    assert st["primary_rays"] == 64 * 48 * 2 and st["shaded_hits"] == 0 and st["shadow_rays"] == 0


def test_create_destroy_does_not_leak_device_memory(hip):
    """The BVH4 nodes and the precomputed triangles (the largest scene buffers) were not freed by rr_scene_destroy."""
    rt = C.CDLL("libamdhip64.so")   # the HIP runtime the library itself is linked against

    def free_bytes():
        free, total = C.c_size_t(0), C.c_size_t(0)
        assert rt.hipDeviceSynchronize() == 0 and rt.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
        return free.value
    fs = load_scene("monkey")
    cam = camera_for(fs, 64, 48).c_struct()
    cfg = make_config(samples=1, monte_carlo=False, seed=0)

    def cycle():
        with hip.DeviceScene(fs, 0) as ds:
            ds.render(cam, cfg)
    cycle()  # first use: code objects, the de-interleave maps, torch's context
    lost = []
    for _ in range(3):   # a leak loses memory in EVERY window; the HIP runtime growing one of its own pools (seen: 16 MiB, once) shows in one
        free0 = free_bytes()
        for _ in range(12):
            cycle()
        lost.append(free0 - free_bytes())
    assert min(lost) < (4 << 20), f"{[round(v / 2**20, 1) for v in lost]} MiB lost over three windows of 12 create / destroy cycles"


def test_material_edits_in_place_equal_a_fresh_scene(hip, oracle):
    fs = load_scene("spheres_room")
    cam = camera_for(fs, 128, 72).c_struct()
    cfg = make_config(samples=2, monte_carlo=True, seed=9)
    edited = copy.deepcopy(fs)
    touched = 0
    for i, it in enumerate(edited.items):   # edit the full material AND its cache, as Material::apply_diff + update_material_cache do
        for idx in (it.material, it.material_cache):
            m = edited.materials[idx]
            if i % 3 == 0:
                m.alpha, m.refraction_index = 0.6, 1.3
            elif i % 3 == 1:
                m.reflectivity, m.base_color = 0.35, (0.9, 0.4, 0.2)
            else:
                m.cast_shadow = False
            touched += 1
    assert touched >= 6
    with hip.DeviceScene(fs, 0) as ds, hip.DeviceScene(edited, 0) as fresh:
        before = ds.render(cam, cfg)
        ds.update_materials(edited.materials)
        after = ds.render(cam, cfg)
        ref = fresh.render(cam, cfg)
        _same(after, ref)
        assert not np.array_equal(before["rgba"], after["rgba"])
        ds.update_materials(fs.materials)   # and back
        _same(ds.render(cam, cfg), before)
        with pytest.raises(hip.RustrayHipError):
            ds.update_materials(edited.materials[:-1])
    res = compare_frames(after, oracle.render(edited.c_struct(), cam, cfg, want_means=True, n_threads=8))
    assert res["n_rgb_over"] == 0 and res["n_id_diff"] == 0, res
    assert_in_band(res)


def test_tuning_is_validated(hip):
    from rustray_amd.flat import rr_tuning
    with hip.DeviceScene(load_scene("spheres"), 0) as ds:
        t = rr_tuning()
        assert hip.lib().rr_scene_set_tuning(ds._h, C.byref(t)) == -1          # struct_size 0
        t.struct_size = C.sizeof(rr_tuning); t.sample_group = 3
        assert hip.lib().rr_scene_set_tuning(ds._h, C.byref(t)) == -1          # not a power of two
        ds.set_tuning(sample_group=4, kernel_timing=1)
        g = rr_tuning()
        assert hip.lib().rr_scene_get_tuning(ds._h, C.byref(g)) == 0 and g.sample_group == 4 and g.kernel_timing == 1


def edit_scene(name):
    """The two scenes of the edit tests: kbert_room (8 items: the per-ray top level) and a fuzzer scene of 42 items (the packet form)."""
    if name == "kbert_room":
        fs = load_scene("kbert_room")
        assert len(fs.items) <= 16
    else:
        from tools.fuzz_parity import rich_scene
        fs = rich_scene(9110)
        assert len(fs.items) >= 17
    return fs


EDIT_SCENES = ["kbert_room", "rich9110"]
EDIT_CFG = dict(samples=2, monte_carlo=True, seed=11)


@pytest.mark.parametrize("name", EDIT_SCENES)
def test_refused_transform_update_leaves_the_scene_as_it_was(hip, name):
    """rr_scene_update_transforms checked each matrix in the loop that wrote it: a NaN in item 3 was refused with items 0..2 already
    holding the new matrices on the host, and the next material update uploaded them without their flat normals and top level."""
    fs = edit_scene(name)
    cam = camera_for(fs, 72, 48).c_struct()
    cfg = make_config(**EDIT_CFG)
    t, ti = item_transforms(fs, 3.0)
    bad = t.copy()
    bad[3, 0, 1] = np.nan
    moved_fs = with_transforms(fs, t, ti)   # (before fs.c_struct(): its ctypes arrays do not deep-copy)
    with hip.DeviceScene(fs, 0) as ds, hip.DeviceScene(moved_fs, 0) as fresh:
        f0 = ds.render(cam, cfg)
        with pytest.raises(hip.RustrayHipError) as e:
            ds.update_transforms(bad, ti)
        assert e.value.code == -1 and "item 3" in str(e.value)
        assert_frames_identical(ds.render(cam, cfg), f0, "after the refused update")
        ds.update_materials(fs.materials)   # a no-op edit: uploads the host's item records
        assert_frames_identical(ds.render(cam, cfg), f0, "after a no-op material update")
        ds.update_transforms(t, ti)
        moved = ds.render(cam, cfg)
        assert_frames_identical(moved, fresh.render(cam, cfg), "moved in place vs a fresh scene")
        assert not np.array_equal(moved["rgba"], f0["rgba"])


def _fault(hip, point, kind, skip=0):
    L = hip.lib()
    L.rr_test_fault.argtypes = [C.c_char_p, C.c_int, C.c_int]
    assert L.rr_test_fault(point.encode(), kind, skip) == 0


@pytest.mark.parametrize("name", EDIT_SCENES)
def test_material_update_failing_between_its_copies_leaves_the_scene_as_it_was(hip, name):
    """A fault between the materials' copy and the items' copy: the materials of before are copied back, the item flags and the
    alpha-occluder hint stay as they were, and the next update works."""
    fs = edit_scene(name)
    cam = camera_for(fs, 72, 48).c_struct()
    cfg = make_config(**EDIT_CFG)
    edited = copy.deepcopy(fs)
    for i, it in enumerate(edited.items):
        for idx in (it.material, it.material_cache):
            m = edited.materials[idx]
            if i % 2 == 0:
                m.alpha = 0.0          # a flag of the item (RR_IF_CACHE_ALPHA_POS) and a material record change together
            else:
                m.base_color, m.cast_shadow = (0.2, 0.8, 0.3), False
    with hip.DeviceScene(fs, 0) as ds, hip.DeviceScene(edited, 0) as fresh:
        f0 = ds.render(cam, cfg)
        try:
            for kind, code in ((1, -5), (2, -4)):
                _fault(hip, "update_materials.device", kind)
                with pytest.raises(hip.RustrayHipError) as e:
                    ds.update_materials(edited.materials)
                assert e.value.code == code, str(e.value)
                assert_frames_identical(ds.render(cam, cfg), f0, f"after a failed material update (kind {kind})")
        finally:
            _fault(hip, "", 0)
        ds.update_materials(edited.materials)
        after = ds.render(cam, cfg)
        assert_frames_identical(after, fresh.render(cam, cfg), "edited in place vs a fresh scene")
        assert not np.array_equal(after["rgba"], f0["rgba"])


def _visible_first(fs, object_id):
    """Item indices, those covering most pixels of the unedited frame first: an edit of an item nobody sees tests nothing."""
    ids, counts = np.unique(np.asarray(object_id), return_counts=True)
    cover = dict(zip(ids.tolist(), counts.tolist()))
    return sorted(range(len(fs.items)), key=lambda i: (-cover.get(fs.items[i].id, 0), i))


def _pick(fs, order, pred):
    for i in order:
        it = fs.items[i]
        if pred(it, fs.materials[it.material], fs.materials[it.material_cache]):
            return i
    raise AssertionError("no item fits the edit")


def _both(fs, i, **kw):
    """Sets fields on an item's full material and its material cache, as Material::apply_diff + update_material_cache do."""
    it = fs.items[i]
    for idx in (it.material, it.material_cache):
        for k, v in kw.items():
            setattr(fs.materials[idx], k, v)


def _shape(t):
    return tuple(np.asarray(t).shape[:2])


def flag_edit_steps(fs, name, case, object_id):
    """The scenes an in-place edit walks through, one per step: every flag item_flags derives from a material, and the material
    record's texture filter and slot.  Each step starts from the one before; the edited item is the most visible one that fits
    (object_id: the unedited frame).  `fs` must not have been through c_struct() (its ctypes arrays do not deep-copy)."""
    cur = copy.deepcopy(fs)
    order = _visible_first(cur, object_id)
    if case == "alpha_map":        # RR_IF_OCCLUDER_ALPHA_TEX and view.any_alpha_occluder, both ways
        caster = _pick(cur, order, lambda it, m, c: c.cast_shadow and it.visible and m.texture[4] < 0)
        amap = int(np.argmin([np.asarray(t)[..., 3].min() for t in cur.textures]))   # the texture with the most transparent texel
        off = copy.deepcopy(cur)
        for m in off.materials:
            m.texture[4] = -1
        if any(m.texture[4] >= 0 for m in cur.materials):   # the rich scene has alpha maps already: clear them, then add one back
            off2on = copy.deepcopy(off)
            off2on.materials[off2on.items[caster].material].texture[4] = amap
            return [off, off2on]
        on = copy.deepcopy(cur)
        on.materials[on.items[caster].material].texture[4] = amap
        return [on, off]
    if case == "cache_alpha_half":   # RR_IF_SOLID_BASE goes with alpha < 1 under backface culling
        i = _pick(cur, order, lambda it, m, c: it.visible and c.alpha == 1.0 and c.backface_cullig)
        _both(cur, i, alpha=0.5)
    elif case == "smooth":           # RR_IF_SMOOTH, on a mesh that has normals
        i = _pick(cur, order, lambda it, m, c: it.visible and it.kind == 1 and cur.meshes[it.mesh].normals is not None
                  and len(cur.meshes[it.mesh].normals) > 0)
        _both(cur, i, smooth_shading=not cur.materials[cur.items[i].material_cache].smooth_shading)
    elif case == "reflection_only":  # RR_IF_CACHE_REFL_ONLY
        i = _pick(cur, order, lambda it, m, c: it.visible and not c.reflection_only)
        _both(cur, i, reflection_only=True)
    elif case == "no_shadow":        # RR_IF_CACHE_CAST_SHADOW
        i = _pick(cur, order, lambda it, m, c: it.visible and c.cast_shadow)
        _both(cur, i, cast_shadow=False)
    elif case == "cache_alpha_zero":  # RR_IF_CACHE_ALPHA_POS
        i = _pick(cur, order, lambda it, m, c: it.visible and c.alpha > 0.0)
        _both(cur, i, alpha=0.0)
    elif case == "filter_and_size":  # the material record: RR_MF_NEAREST and a texture descriptor of another size
        i = _pick(cur, order, lambda it, m, c: it.visible and m.texture[0] >= 0)
        m = cur.materials[cur.items[i].material]
        old = _shape(cur.textures[m.texture[0]])
        others = [k for k, t in enumerate(cur.textures) if _shape(t) != old]
        if name != "kbert_room":
            others = [k for k in others if any(v & (v - 1) for v in _shape(cur.textures[k]))] or others
        m.texture[0] = others[0]
        m.texture_filtering_nearest = not m.texture_filtering_nearest
    else:
        raise ValueError(case)
    return [cur]


def frames_differ(a, b):
    return any(not np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8))
               for k in ("rgba", "depth", "normal", "object_id"))


FLAG_CASES = ["alpha_map", "cache_alpha_half", "smooth", "reflection_only", "no_shadow", "cache_alpha_zero", "filter_and_size"]


@pytest.mark.parametrize("case", FLAG_CASES)
@pytest.mark.parametrize("name", EDIT_SCENES)
def test_material_flag_edits_in_place_equal_a_fresh_scene_and_the_oracle(hip, oracle, name, case):
    fs = edit_scene(name)
    work = copy.deepcopy(fs)   # edited copies are made from this one (fs goes through c_struct() below)
    cam = camera_for(fs, 72, 48).c_struct()
    cfg = make_config(samples=2, monte_carlo=True, seed=5)
    with hip.DeviceScene(fs, 0) as ds:
        prev = ds.render(cam, cfg)
        for k, edited in enumerate(flag_edit_steps(work, name, case, prev["object_id"])):
            ds.update_materials(edited.materials)
            got = ds.render(cam, cfg)
            st = ds.stats()
            assert frames_differ(got, prev), f"{case} step {k}: the edit does not change the frame, so it tests nothing"
            with hip.DeviceScene(edited, 0) as fresh:
                assert_frames_identical(got, fresh.render(cam, cfg), f"{case} step {k}: in place vs a fresh scene")
            ref = oracle.render(edited.c_struct(), cam, cfg, want_means=True, n_threads=8, want_counters=True)
            res = compare_frames(got, ref)
            assert res["n_rgb_over"] == 0 and res["n_id_diff"] == 0, (case, k, res)
            assert_in_band(res, f"{case} {k}")
            c = ref["counters"]
            assert (st["primary_rays"], st["secondary_rays"], st["shaded_hits"]) == (c["rays_primary"], c["rays_secondary"], c["shaded_hits"]), (case, k)
            prev = got
