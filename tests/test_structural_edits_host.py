"""Structural scene edits without a GPU: plan_scene_update(..., structural=True) for the GUI's object "delete", "add ground plane" and
"add environment sphere" (rustray_amd/renderer.py), the Scene mirrors of the two "add" actions on the fixture tree
tests/golden/add_objects (rustray_amd/scene.py), and the two ABI entry points rr_scene_add_meshes / rr_scene_set_items as far as
they go without a device (exported, NULL arguments refused, both definitions guarded)."""
import copy
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from rustray_amd import capi
from rustray_amd.flat import RR_ITEM_MESH, RR_ITEM_SPHERE, TEX_NAMES
from rustray_amd.renderer import IN_PLACE_STEPS, RECREATE, STRUCTURAL_STEPS, Raytracing, _resident_mesh_indices, plan_scene_update
from rustray_amd.scene import Scene, scene_from_flat
from tests.helpers import GOLDEN, ROOT, host_api_source, load_scene

FIXTURE = os.path.join(GOLDEN, "add_objects")


def scene_of(fs, root=FIXTURE) -> Scene:
    """The flat scene as a Scene over the fixture tree, so that the GUI actions of rustray_amd/scene.py can run on a fixture scene."""
    return scene_from_flat(fs, root)


@pytest.fixture(scope="module")
def base():
    fs = scene_of(load_scene("kbert_room")).flatten()
    assert len(fs.items) >= 4 and len(fs.textures) >= 1 and len(fs.meshes) >= 2
    return fs


def flat_after(fs, action):
    sc = scene_of(fs)
    action(sc)
    return sc.flatten()


# ---- the planner -------------------------------------------------------------------------------------------------------------------
def test_constants_and_defaults_are_pinned():
    assert STRUCTURAL_STEPS == ("add_textures", "add_meshes", "set_items", "update_lights")
    assert IN_PLACE_STEPS == ("add_textures", "update_materials", "update_transforms", "update_item_flags", "update_lights")
    assert inspect.signature(plan_scene_update).parameters["structural"].default is False
    assert inspect.signature(Raytracing.apply_scene).parameters["structural"].default is False


def test_delete_is_set_items(base):
    new = flat_after(base, lambda sc: sc.delete_object_by_id(base.items[2].id))
    assert len(new.items) == len(base.items) - 1
    assert plan_scene_update(base, new, structural=True) == ["set_items"]
    assert plan_scene_update(base, new) == [RECREATE]                        # the default mode is what it was
    assert plan_scene_update(base, new, structural=False) == [RECREATE]


def test_a_deleted_items_orphaned_mesh_is_no_edit(base):
    """The mesh of a deleted item stays in the flat scene's list, unnamed (Scene.flatten() keeps every mesh): that is no edit.  A flat
    scene that dropped the mesh asks for a new handle: meshes are never removed from a resident one."""
    victim = next(it for it in base.items if it.kind == RR_ITEM_MESH and sum(o.mesh == it.mesh for o in base.items) == 1)
    keeps = flat_after(base, lambda sc: sc.delete_object_by_id(victim.id))
    assert len(keeps.meshes) == len(base.meshes)
    assert plan_scene_update(base, keeps, structural=True) == ["set_items"]
    drops = copy.deepcopy(keeps)
    del drops.meshes[victim.mesh]
    for it in drops.items:
        if it.mesh > victim.mesh:
            it.mesh -= 1
    assert plan_scene_update(base, drops, structural=True) == [RECREATE]
    index, appended = _resident_mesh_indices(base.meshes, drops.meshes)
    assert appended == [] and index == [k for k in range(len(base.meshes)) if k != victim.mesh]


def test_ground_plane_is_add_meshes_then_set_items(base):
    new = flat_after(base, Scene.add_ground_plane)
    assert len(new.items) == len(base.items) + 1 and len(new.meshes) == len(base.meshes) + 1 and len(new.textures) == len(base.textures)
    assert plan_scene_update(base, new, structural=True) == ["add_meshes", "set_items"]
    assert plan_scene_update(base, new) == [RECREATE]
    # once the plane's mesh is resident, a second plane of the same content needs no mesh
    again = flat_after(new, Scene.add_ground_plane)
    assert len(again.meshes) == len(new.meshes) + 1
    assert plan_scene_update(new, again, structural=True) == ["set_items"]


def test_environment_sphere_is_add_textures_then_set_items(base):
    new = flat_after(base, Scene.add_environment_sphere)
    assert len(new.items) == len(base.items) + 1 and len(new.meshes) == len(base.meshes) and len(new.textures) == len(base.textures) + 1
    assert plan_scene_update(base, new, structural=True) == ["add_textures", "set_items"]
    assert plan_scene_update(base, new) == [RECREATE]
    both = flat_after(new, Scene.add_ground_plane)
    both.lights[0].intensity *= 2.0
    assert plan_scene_update(base, both, structural=True) == ["add_textures", "add_meshes", "set_items", "update_lights"]


def test_a_changed_resident_texture_recreates(base):
    new = flat_after(base, lambda sc: sc.delete_object_by_id(base.items[0].id))
    new.textures[0] = new.textures[0].copy()
    new.textures[0][0, 0, 0] ^= 1
    assert plan_scene_update(base, new, structural=True) == [RECREATE]
    gone = flat_after(base, lambda sc: sc.delete_object_by_id(base.items[0].id))
    gone.textures.pop()
    assert plan_scene_update(base, gone, structural=True) == [RECREATE]


def test_a_changed_resident_mesh_recreates(base):
    """Meshes are recognised by content: an edited vertex makes a mesh the device does not hold and leaves one it holds without a
    counterpart.  Kept next to its edited copy, the old mesh stays resident and the copy is appended."""
    new = copy.deepcopy(base)
    k = next(it.mesh for it in new.items if it.kind == RR_ITEM_MESH)
    new.meshes[k].positions = np.asarray(new.meshes[k].positions, np.float32).copy()
    new.meshes[k].positions[0, 1] += 0.25
    assert plan_scene_update(base, new) == [RECREATE]
    assert plan_scene_update(base, new, structural=True) == [RECREATE]
    index, appended = _resident_mesh_indices(base.meshes, new.meshes)
    assert len(appended) == 1 and index[k] == len(base.meshes) and all(index[j] == j for j in range(len(base.meshes)) if j != k)
    new.meshes.append(base.meshes[k])
    assert plan_scene_update(base, new, structural=True) == ["add_meshes", "set_items"]


def test_mesh_indices_are_remapped_by_content(base):
    new = copy.deepcopy(base)
    new.meshes.reverse()                                    # the same meshes, listed the other way round
    n = len(new.meshes)
    for it in new.items:
        if it.mesh >= 0:
            it.mesh = n - 1 - it.mesh
    assert plan_scene_update(base, new, structural=True) == ["set_items"]
    index, appended = _resident_mesh_indices(base.meshes, new.meshes)
    assert appended == []
    for old, it in zip(base.items, new.items):
        if it.mesh >= 0:
            assert index[it.mesh] == old.mesh
    # what the device holds may be more than the flat scene of creation lists
    plane = flat_after(base, Scene.add_ground_plane)
    resident = list(base.meshes) + [plane.meshes[-1]]
    assert plan_scene_update(base, plane, structural=True, resident_meshes=resident) == ["set_items"]
    assert _resident_mesh_indices(resident, plane.meshes)[0][-1] == len(base.meshes)


def test_nothing_structural_gives_the_default_plan(base):
    same = copy.deepcopy(base)
    assert plan_scene_update(base, same, structural=True) == [] == plan_scene_update(base, same)
    same.lights[0].intensity *= 0.5
    same.items[1].visible = not same.items[1].visible
    same.items[2].trans = np.asarray(same.items[2].trans, np.float32).copy()
    same.items[2].trans[0, 3] += 1.0
    same.materials[0].reflectivity = 0.25
    want = ["update_materials", "update_transforms", "update_item_flags", "update_lights"]
    assert plan_scene_update(base, same) == want and plan_scene_update(base, same, structural=True) == want


# ---- the Scene mirrors -------------------------------------------------------------------------------------------------------------
def _bottom_y_f64(fs):
    lo = np.inf
    for it in fs.items:
        t = np.asarray(it.trans, np.float64)
        for k in range(8):
            c = [(it.bbox_max if k & (1 << a) else it.bbox_min)[a] for a in range(3)]
            lo = min(lo, float(t[1, :3] @ np.asarray(c, np.float64) + t[1, 3]))
    return lo


def test_find_bottom_y_pos_is_the_lowest_box_corner_in_f32(base):
    sc = scene_of(base)
    y = sc.find_bottom_y_pos()
    assert y == float(np.float32(y))
    want = _bottom_y_f64(base)
    scale = max(abs(np.asarray(it.trans, np.float64)[1]).sum() * max(np.abs(it.bbox_min).max(), np.abs(it.bbox_max).max(), 1.0) for it in base.items)
    assert abs(y - want) <= 4 * 2.0 ** -24 * scale, (y, want)      # three f32 products and three f32 sums per corner
    assert Scene(FIXTURE).find_bottom_y_pos() == float(np.finfo(np.float32).max)   # std::f32::MAX for a scene without items
    one = Scene(FIXTURE)
    one.add_environment_sphere()
    assert one.find_bottom_y_pos() == -100.0


def test_ground_plane_lands_on_the_lowest_point(base):
    sc = scene_of(base)
    y = sc.find_bottom_y_pos()
    next_id = sc.item_id
    ids = sc.add_ground_plane()
    plane = sc.items[-1]
    assert plane.name == "floor reflective" and plane.kind == RR_ITEM_MESH and ids == [next_id + 2]
    assert plane.id == next_id + 3                      # the material takes an id, and the item's id is assigned twice (src/scene.rs:541)
    want = np.eye(4, dtype=np.float32)
    want[1, 3] = np.float32(y)
    assert np.array_equal(plane.trans, want)
    assert abs(float(plane.trans[1, 3]) - _bottom_y_f64(base)) <= 1e-5 * max(1.0, abs(_bottom_y_f64(base)))
    m = sc.meshes[plane.mesh]
    assert np.array_equal(m.positions, np.asarray([[-10000, 0, 10000], [10000, 0, 10000], [10000, 0, -10000], [-10000, 0, -10000]], np.float32))
    assert np.array_equal(m.indices, [[0, 1, 2], [0, 2, 3]]) and len(m.uvs) == 4 and len(m.normals) == 0
    mat = sc.materials[plane.material_id]
    f = np.float32
    assert mat.base_color == (float(f(0.2)),) * 3 and mat.specular_color == (float(f(0.2) * f(0.8)),) * 3 and mat.ambient_color == (0.0, 0.0, 0.0)
    assert mat.reflectivity == float(f(0.8)) and mat.roughness == float(f(0.015)) and mat.alpha == 1.0
    assert mat.texture == [-1] * 8 and mat.cast_shadow and mat.receive_shadow and not mat.reflection_only and mat.backface_cullig
    # the plane is part of the scene it is measured in the next time: a second one lands where the first one lies, and it is the
    # FIRST item of that name that is moved (Scene::get_by_name_mut), as in the reference
    sc.add_ground_plane()
    assert float(sc.items[-2].trans[1, 3]) == float(np.float32(np.float32(y) + np.float32(y))) and float(sc.items[-1].trans[1, 3]) == 0.0


def test_environment_sphere_is_reflection_only_with_its_ambient_map(base):
    sc = scene_of(base)
    n_tex = len(sc.textures)
    sc.add_environment_sphere()
    env = sc.items[-1]
    assert env.name == "environment" and env.kind == RR_ITEM_SPHERE and env.radius == 100.0 and env.mesh is None
    assert np.array_equal(env.trans, np.eye(4, dtype=np.float32)) and env.visible and not env.flip_normals
    mat = sc.materials[env.material_id]
    assert mat.reflection_only and not mat.backface_cullig and mat.base_color == (0.0, 0.0, 0.0) and mat.ambient_color == (1.0, 1.0, 1.0)
    slot = TEX_NAMES.index("ambient")
    assert mat.texture[slot] == n_tex and all(t == -1 for k, t in enumerate(mat.texture) if k != slot)
    assert len(sc.textures) == n_tex + 1 and sc.textures[-1].shape == (32, 64, 4) and (sc.textures[-1][..., 3] == 255).all()
    assert sc.material_tex_paths[env.material_id] == {slot: "scene/textures/environment/footprint_court.jpg"}
    fs = sc.flatten()
    it = fs.items[-1]
    assert fs.materials[it.material].texture[slot] == n_tex and fs.materials[it.material_cache].texture == [-1] * 8
    assert fs.materials[it.material_cache].reflection_only and it.bbox_min == (-100.0,) * 3 and it.bbox_max == (100.0,) * 3
    sc.add_environment_sphere()                          # the image is loaded once
    assert len(sc.textures) == n_tex + 1 and sc.materials[sc.items[-1].material_id].texture[slot] == n_tex


def test_fixture_tree_holds_data_only():
    found = sorted(os.path.relpath(os.path.join(d, f), FIXTURE) for d, _, fs in os.walk(FIXTURE) for f in fs if "__pycache__" not in d)
    assert found == ["make_add_objects.py", "scene/environment.json", "scene/floor_reflective.json", "scene/textures/environment/footprint_court.jpg"]
    from PIL import Image
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_add_objects", os.path.join(FIXTURE, "make_add_objects.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    im = np.asarray(Image.open(os.path.join(FIXTURE, found[-1])).convert("RGB"), np.int32)
    assert im.shape == (32, 64, 3) and np.abs(im - mod.stand_in().astype(np.int32)).mean() < 6.0   # the generated stand-in, through JPEG


# ---- the ABI, as far as it goes without a device --------------------------------------------------------------------------------------
def test_both_symbols_are_exported_and_refuse_null():
    assert "rr_scene_add_meshes" in capi.EXPORTS and "rr_scene_set_items" in capi.EXPORTS
    L = capi.lib()
    assert hasattr(L, "rr_scene_add_meshes") and hasattr(L, "rr_scene_set_items")
    first = C.c_uint32(77)
    assert L.rr_scene_add_meshes(None, None, 0, C.byref(first)) == -1 and first.value == 77
    assert b"NULL" in L.rr_last_error()
    assert L.rr_scene_set_items(None, None, 0, None, 0) == -1
    assert b"NULL" in L.rr_last_error()
    assert L.rr_abi_version() == 3
    with open(os.path.join(ROOT, "include", "rustray_hip.h")) as f:
        hdr = f.read()
    assert "#define RR_ABI_VERSION 3u" in hdr
    assert re.search(r"int rr_scene_add_meshes\(rr_scene\* scene, const rr_mesh\* meshes, uint32_t n_meshes, uint32_t\* first_index\);", hdr)
    assert re.search(r"int rr_scene_set_items\(rr_scene\* scene, const rr_item\* items, uint32_t n_items,\s*const rr_material\* materials, uint32_t n_materials\);", hdr)
    assert "rr_scene_add_meshes and rr_scene_set_items" in hdr.split("#define RR_ABI_VERSION")[0]   # the symbols a version-3 library may lack


def test_both_definitions_are_guarded_and_commit_last():
    src = host_api_source()
    for name, point in (("rr_scene_add_meshes", "add_meshes.device"), ("rr_scene_set_items", "set_items.device")):
        m = re.search(r'extern "C" int ' + name + r"\([^)]*\) try \{(.*?)\} RR_GUARD_END\(\"" + name + r"\"\)", src, re.S)
        assert m, f"{name} is not a function-try-block closed by RR_GUARD_END"
        body = m.group(1)
        assert f'not_in_pass(s, "{name}")' in body and "std::lock_guard<std::mutex> lk(s->mu)" in body
        # nothing of the scene is written before the fault point and the wait for frames in flight; no "broken" flag is involved
        head, tail = body.split(f'RR_FAULT_POINT("{point}")')
        assert "hipDeviceSynchronize()" in tail.split("commit")[0]
        assert not re.search(r"\bs->(?!mu\b)\w+(\.\w+)*\s*(=[^=]|\.swap|\.push_back)", head.replace("s->data.h_meshes.reserve", "")), name
        assert "broken_" not in body and "all_or_nothing" not in body
    m = re.search(r"static int check_intact\(const rr_scene\* s\) \{(.*?)\n\}", src, re.S)
    assert sorted(set(re.findall(r"broken_\w+", m.group(1)))) == ["broken_geometry", "broken_item_flags", "broken_lights", "broken_materials"]
