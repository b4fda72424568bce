"""Raytracing.apply_scene's choice without a GPU: plan_scene_update (rustray_amd/renderer.py) against every kind of difference between
the flat scene a handle was created from and the edited one, and the GUI deletes of rustray_amd/scene.py."""
import copy

import numpy as np
import pytest

from rustray_amd.flat import RR_LIGHT_SPOT, Light
from rustray_amd.renderer import IN_PLACE_STEPS, RECREATE, plan_scene_update
from rustray_amd.scene import Scene
from tests.helpers import load_scene


@pytest.fixture(scope="module")
def base():
    fs = load_scene("kbert_room")
    assert len(fs.items) >= 2 and len(fs.textures) >= 1 and len(fs.lights) >= 2 and len(fs.meshes) >= 1
    return fs


def edited(fs, fn):
    out = copy.deepcopy(fs)
    fn(out)
    return out


def test_no_difference_is_an_empty_plan(base):
    assert plan_scene_update(base, copy.deepcopy(base)) == []
    assert plan_scene_update(base, base) == []


def _set_light(**kw):
    def f(fs):
        for k, v in kw.items():
            setattr(fs.lights[1], k, v)
    return f


@pytest.mark.parametrize("fn", [
    _set_light(pos=(1.0, 2.0, 3.0)), _set_light(dir=(0.0, 0.0, -1.0)), _set_light(color=(0.2, 0.3, 0.4)), _set_light(intensity=17.0),
    _set_light(max_angle=0.3), _set_light(light_type=RR_LIGHT_SPOT), _set_light(enabled=False),
    lambda fs: fs.lights.append(Light()),                  # light "+"
    lambda fs: fs.lights.pop(0),                           # light "delete"
    lambda fs: fs.lights.clear(),
], ids=["pos", "dir", "color", "intensity", "max_angle", "type", "enabled", "add", "delete", "none"])
def test_light_edits_update_the_lights(base, fn):
    assert plan_scene_update(base, edited(base, fn)) == ["update_lights"]


def test_light_id_alone_is_no_edit(base):
    """Light::id names a light for the GUI; it does not cross the ABI."""
    assert plan_scene_update(base, edited(base, _set_light(id=12345))) == []


@pytest.mark.parametrize("field", ["visible", "flip_normals"])
def test_item_flag_edits_update_the_item_flags(base, field):
    def f(fs):
        setattr(fs.items[1], field, not getattr(fs.items[1], field))
    assert plan_scene_update(base, edited(base, f)) == ["update_item_flags"]


def test_transform_edit_updates_the_transforms(base):
    def f(fs):
        fs.items[0].trans = fs.items[0].trans.copy(); fs.items[0].trans[0, 3] += 1.0
    assert plan_scene_update(base, edited(base, f)) == ["update_transforms"]

    def g(fs):
        fs.items[0].trans_inv = fs.items[0].trans_inv.copy(); fs.items[0].trans_inv[1, 3] -= 0.5
    assert plan_scene_update(base, edited(base, g)) == ["update_transforms"]


def test_material_edit_updates_the_materials(base):
    assert plan_scene_update(base, edited(base, lambda fs: setattr(fs.materials[0], "alpha", 0.25))) == ["update_materials"]
    assert plan_scene_update(base, edited(base, lambda fs: fs.materials[0].texture.__setitem__(0, -1 if fs.materials[0].texture[0] >= 0 else 0))) == ["update_materials"]


def test_new_texture_is_added_then_named(base):
    img = np.full((4, 8, 4), 200, np.uint8)

    def f(fs):
        fs.textures.append(img)
        fs.materials[0].texture[0] = len(fs.textures) - 1
    assert plan_scene_update(base, edited(base, f)) == ["add_textures", "update_materials"]
    assert plan_scene_update(base, edited(base, lambda fs: fs.textures.append(img))) == ["add_textures"]


def _negate(fs, attr):
    """Negates `attr` of the first mesh that has any."""
    m = next(m for m in fs.meshes if len(getattr(m, attr)) and np.abs(getattr(m, attr)).max() > 0)
    setattr(m, attr, -np.asarray(getattr(m, attr)))


@pytest.mark.parametrize("fn", [
    lambda fs: fs.items.pop(1),                                                    # object "delete"
    lambda fs: fs.items.append(copy.deepcopy(fs.items[0])),                        # ground plane / environment sphere
    lambda fs: setattr(fs.items[1], "kind", 1 - fs.items[1].kind),
    lambda fs: setattr(fs.items[1], "id", fs.items[1].id + 1000),
    lambda fs: setattr(fs.items[1], "mesh", (fs.items[1].mesh + 1) % len(fs.meshes)),
    lambda fs: setattr(fs.items[1], "material", (fs.items[1].material + 1) % len(fs.materials)),
    lambda fs: setattr(fs.items[1], "material_cache", (fs.items[1].material_cache + 1) % len(fs.materials)),
    lambda fs: setattr(fs.items[1], "radius", fs.items[1].radius + 1.0),
    lambda fs: setattr(fs.items[1], "bbox_min", (-9.0, -9.0, -9.0)),
    lambda fs: setattr(fs.items[1], "bbox_max", (9.0, 9.0, 9.0)),
    lambda fs: setattr(fs.meshes[0], "positions", fs.meshes[0].positions * np.float32(1.5)),
    lambda fs: setattr(fs.meshes[0], "indices", fs.meshes[0].indices[::-1].copy()),
    lambda fs: _negate(fs, "uvs"),
    lambda fs: _negate(fs, "normals"),
    lambda fs: fs.meshes.append(copy.deepcopy(fs.meshes[0])),
    lambda fs: fs.materials.append(copy.deepcopy(fs.materials[0])),
    lambda fs: fs.materials.pop(),
    lambda fs: fs.textures.__setitem__(0, 255 - fs.textures[0]),                  # an existing image changed
    lambda fs: fs.textures.__setitem__(0, fs.textures[0][:-1].copy()),            # ... or its size
    lambda fs: fs.textures.pop(),                                                  # the list got shorter
], ids=["delete_item", "add_item", "kind", "id", "mesh_index", "material_index", "cache_index", "radius", "bbox_min", "bbox_max",
        "mesh_positions", "mesh_indices", "mesh_uvs", "mesh_normals", "mesh_count", "material_count_up", "material_count_down",
        "texture_pixels", "texture_size", "texture_count_down"])
def test_structural_edits_recreate(base, fn):
    assert plan_scene_update(base, edited(base, fn)) == [RECREATE]


def test_combined_edits_run_in_order(base):
    img = np.zeros((2, 2, 4), np.uint8)

    def f(fs):
        fs.lights[0].intensity *= 2.0
        fs.items[0].visible = not fs.items[0].visible
        fs.items[1].trans = fs.items[1].trans.copy(); fs.items[1].trans[2, 3] += 0.5
        fs.materials[1].base_color = (0.1, 0.2, 0.3)
        fs.textures.append(img)
    assert plan_scene_update(base, edited(base, f)) == list(IN_PLACE_STEPS)


@pytest.mark.parametrize("second", [
    lambda fs: fs.items.pop(0),
    lambda fs: fs.materials.append(copy.deepcopy(fs.materials[0])),
    lambda fs: setattr(fs.meshes[0], "positions", fs.meshes[0].positions + np.float32(1.0)),
], ids=["item_deleted", "material_added", "mesh_changed"])
def test_any_structural_edit_beside_in_place_ones_recreates(base, second):
    def f(fs):
        fs.lights[0].color = (0.5, 0.5, 0.5)           # in place on its own ...
        fs.items[-1].flip_normals = True
        second(fs)                                      # ... but not beside this
    assert plan_scene_update(base, edited(base, f)) == [RECREATE]


def test_gui_deletes_mirror_the_reference():
    """Scene::delete_light_by_id / delete_object_by_id (src/scene.rs:1580-1620): the last entry with the id goes, later ones move up;
    an unknown id changes nothing.  Lights get ids from the same counter as items (add_default_light, src/scene.rs:1386-1401)."""
    sc = Scene()
    for _ in range(3):
        sc.add_default_light()
    ids = [l.id for l in sc.lights]
    assert ids == [1, 2, 3]
    sc.lights[2].intensity = 5.0
    sc.delete_light_by_id(2)
    assert [l.id for l in sc.lights] == [1, 3] and sc.lights[1].intensity == 5.0
    sc.delete_light_by_id(99)
    assert [l.id for l in sc.lights] == [1, 3]

    class Obj:
        def __init__(self, i):
            self.id = i
    sc.items = [Obj(4), Obj(5), Obj(6), Obj(5)]
    sc.delete_object_by_id(5)
    assert [o.id for o in sc.items] == [4, 5, 6]
    sc.delete_object_by_id(42)
    assert [o.id for o in sc.items] == [4, 5, 6]
