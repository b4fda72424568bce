"""The edit sequences of tests/test_gpu_structural_edits.py and the bookkeeping of a live handle under them: flat scenes that differ in
their item, material, mesh and texture lists, each step starting from the one before.  No device is needed to make them."""
from __future__ import annotations

import copy

import numpy as np

from rustray_amd.flat import RR_ITEM_MESH, RR_ITEM_SPHERE, FlatScene, Item, Material
from rustray_amd.renderer import _resident_mesh_indices
from rustray_amd.scene import Scene, flat_scene_after_add, inverse_affine
from tests.test_structural_edits_host import FIXTURE


def flat_add(fs: FlatScene, action) -> FlatScene:
    """`fs` after a GUI "add" action of rustray_amd/scene.py, with the scene files of tests/golden/add_objects."""
    return flat_scene_after_add(fs, action, FIXTURE)


def moved_copy(it: Item, new_id: int, offset, name: str) -> Item:
    """A second instance of the item's mesh (or ball): the same local geometry under a transform moved by `offset`."""
    d = copy.deepcopy(it)
    t = np.asarray(it.trans, np.float64).copy()
    t[:3, 3] += np.asarray(offset, np.float64)
    d.trans = t.astype(np.float32)
    d.trans_inv = inverse_affine(d.trans)
    d.id, d.name, d.visible = new_id, name, True
    return d


def coverage(fs: FlatScene, object_id) -> list:
    ids, counts = np.unique(np.asarray(object_id), return_counts=True)
    cover = dict(zip(ids.tolist(), counts.tolist()))
    return [cover.get(it.id, 0) for it in fs.items]


def structural_steps(work: FlatScene, first_object_id, go_to_16: bool):
    """(name, scene) per step; `first_object_id`: the object ids of the unedited scene's frame (which items are seen, and how much)."""
    cur = copy.deepcopy(work)
    cover = coverage(cur, first_object_id)
    next_id = max(it.id for it in cur.items) + 100
    steps = []
    most = max(range(len(cur.items)), key=lambda i: (cover[i], -i))
    del cur.items[most]
    steps.append(("delete_most_visible", copy.deepcopy(cur)))
    del cur.items[-1]
    steps.append(("delete_last", copy.deepcopy(cur)))
    cur = flat_add(cur, Scene.add_ground_plane)
    steps.append(("add_ground_plane", copy.deepcopy(cur)))
    cur = flat_add(cur, Scene.add_environment_sphere)
    steps.append(("add_environment_sphere", copy.deepcopy(cur)))
    cover_now = {it.id: c for it, c in zip(work.items, cover)}
    src = max((it for it in cur.items if it.kind == RR_ITEM_MESH and it.visible and cover_now.get(it.id, 0) > 0 and len(cur.meshes[it.mesh].indices) > 2),
              key=lambda it: cover_now[it.id])
    size = np.asarray(src.bbox_max, np.float64) - np.asarray(src.bbox_min, np.float64)
    scale = np.abs(np.asarray(src.trans, np.float64)[:3, :3]).sum(axis=1)
    cur.items.insert(len(cur.items) // 2, moved_copy(src, next_id, (0.35 * size[0] * scale[0], 0.3 * size[1] * scale[1], 0.2 * size[2] * scale[2]), "second_instance"))
    steps.append(("second_instance", copy.deepcopy(cur)))
    cur.items.reverse()
    steps.append(("reversed", copy.deepcopy(cur)))
    full = copy.deepcopy(cur)
    if go_to_16:
        seen = {it.id: c for it, c in zip(work.items, cover)}
        order = sorted(range(len(cur.items)), key=lambda i: (-seen.get(cur.items[i].id, 1 << 30), i))   # the added items first, then by coverage
        keep17 = sorted(order[:17])
        keep16 = sorted(order[:16])
        cur.items = [full.items[i] for i in keep16]
        steps.append(("down_to_16", copy.deepcopy(cur)))
        cur.items = [full.items[i] for i in keep17]
        steps.append(("back_to_17", copy.deepcopy(cur)))
    cur.items = []
    steps.append(("no_items", copy.deepcopy(cur)))
    cur = copy.deepcopy(full)
    steps.append(("everything_back", copy.deepcopy(cur)))
    return steps


def marker_ball(fs: FlatScene, eye, towards, k: int, new_id: int, radius: float) -> FlatScene:
    """`fs` with one more small ball in front of the camera (the k-th of a 4-wide grid across the view), with a material pair of its
    own: an item that is certainly seen."""
    out = copy.deepcopy(fs)
    eye, towards = np.asarray(eye, np.float64), np.asarray(towards, np.float64)
    fwd = towards / np.linalg.norm(towards)
    right = np.cross(fwd, (0.0, 1.0, 0.0)); right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    pos = eye + fwd * (12.0 * radius) + right * ((k % 4) - 1.5) * 3.0 * radius + up * ((k // 4) - 1.0) * 3.0 * radius
    m = Material(base_color=(0.9 - 0.05 * k, 0.2 + 0.05 * k, 0.3), reflectivity=0.2 if k % 2 else 0.0)
    out.materials += [m, Scene._cache_of(m)]
    t = np.eye(4, dtype=np.float32)
    t[:3, 3] = pos.astype(np.float32)
    out.items.append(Item(kind=RR_ITEM_SPHERE, id=new_id, material=len(out.materials) - 2, material_cache=len(out.materials) - 1, radius=radius,
                          trans=t, trans_inv=inverse_affine(t), bbox_min=(-radius,) * 3, bbox_max=(radius,) * 3, name=f"marker_{k}"))
    return out


class Live:
    """A resident handle and what it holds: the meshes in resident order and the number of images.  `goto(new)` brings it to the
    flat scene `new` through rr_scene_add_textures / rr_scene_add_meshes / rr_scene_set_items (lights are not edited here)."""

    def __init__(self, hip, fs: FlatScene, device: int = 0):
        self.ds = hip.DeviceScene(copy.deepcopy(fs), device)
        self.meshes = list(fs.meshes)
        self.n_textures = len(fs.textures)

    def resident_items(self, new: FlatScene):
        index, appended = _resident_mesh_indices(self.meshes, new.meshes)
        items = [copy.copy(it) for it in new.items]
        for it in items:
            if it.mesh >= 0:
                it.mesh = index[it.mesh]
        return items, appended

    def goto(self, new: FlatScene):
        if len(new.textures) > self.n_textures:
            assert self.ds.add_textures(new.textures[self.n_textures:]) == self.n_textures
            self.n_textures = len(new.textures)
        items, appended = self.resident_items(new)
        if appended:
            assert self.ds.add_meshes(appended) == len(self.meshes)
            self.meshes += appended
        self.ds.set_items(items, new.materials)

    def close(self):
        self.ds.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
