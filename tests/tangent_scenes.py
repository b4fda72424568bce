"""The scene of tests/test_gpu_tangent_frames.py (and of tests/golden/make_tangent_frames.py, which recorded its surface query):
normal-mapped quads whose tangent frame comes from DSceneView::flat_normals -- a plane with the normal on the y axis (the z fallback
of the tangent), two tilted just off it (5e-5 rad: |normal x y| below the 0.0001 of the fallback; 3e-4 rad: above), one seen from its
back, one with flipped normals, one rotated and scaled non-uniformly -- beside a smooth-shaded normal-mapped quad (the per-hit frame)
and a quad without a normal map, which a texture edit gives one."""
import numpy as np

from rustray_amd.flat import FlatScene, Item, Light, Material
from rustray_amd.scene import Scene, get_transformation, inverse_affine
from tests import corner_scenes as cs

NORMAL_SLOT = 3
# name -> (mesh, translation, scale, rotation, flip_normals, smooth, backface culling, normal map)
PARTS = {
    "on_y":       (0, (-3.3, 0.0, -1.2), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), False, False, True, True),
    "off_y_5e-5": (0, (-1.1, 0.0, -1.2), (1.0, 1.0, 1.0), (5e-5, 0.0, 0.0), False, False, True, True),
    "off_y_3e-4": (0, (1.1, 0.0, -1.2), (1.0, 1.0, 1.0), (3e-4, 0.0, 0.0), False, False, True, True),
    "back":       (0, (3.3, 0.3, -1.2), (1.0, 1.0, 1.0), (np.pi - 0.3, 0.0, 0.0), False, False, False, True),
    "flipped":    (0, (-3.3, 0.2, 1.2), (1.0, 1.0, 1.0), (0.4, 0.0, 0.1), True, False, True, True),
    "turned":     (0, (-1.1, 0.3, 1.2), (1.2, 0.5, 0.8), (0.5, 0.7, 0.2), False, False, True, True),
    "smooth":     (1, (1.1, 0.2, 1.2), (1.0, 1.0, 1.0), (0.2, 0.0, -0.2), False, True, True, True),
    "plain":      (0, (3.3, 0.2, 1.2), (1.0, 1.0, 1.0), (0.1, 0.3, 0.3), False, False, True, False),
}
EXTRA = (0, (0.0, 1.2, 0.0), (0.6, 1.0, 0.6), (0.9, 0.2, 0.0), False, False, True, True)   # the item a structural edit adds


def _item(fs, name, part, idn, turn, attach):
    mesh, t, s, r, flip, smooth, cull, mapped = part
    m = Material(base_color=(0.8, 0.7, 0.6), specular_color=(0.6, 0.6, 0.6), shininess=20.0, roughness=0.02 if name == "turned" else 0.0,
                 smooth_shading=smooth, backface_cullig=cull, normal_map_strength=1.0 if name != "off_y_3e-4" else 0.4)
    if mapped or attach:
        m.texture[NORMAL_SLOT] = 0
    mi, ci = cs._mat(fs, m)
    trans = get_transformation(np.eye(4, dtype=np.float32), t, s, r)
    if turn:
        trans = get_transformation(trans, (0.0, 0.05, 0.0), (1.0, 1.0, 1.0), (0.15, 0.25, -0.1))
    p = fs.meshes[mesh].positions
    fs.items.append(Item(kind=1, id=idn, material=mi, material_cache=ci, mesh=mesh, trans=trans, trans_inv=inverse_affine(trans),
                         bbox_min=tuple(p.min(0)), bbox_max=tuple(p.max(0)), flip_normals=flip, name=name))


def scene(turn=False, edit_items=False, attach=False):
    """`turn`: every item turned (rr_scene_update_transforms); `edit_items`: "on_y" deleted, "off_y_3e-4" replaced by a steeper one, one
    item added (rr_scene_set_items); `attach`: "plain" gets the normal map (rr_scene_update_materials)."""
    fs = FlatScene()
    rng = np.random.default_rng(5)
    nm = np.full((8, 8, 4), 255, np.uint8)
    nm[..., :2] = rng.integers(50, 206, (8, 8, 2)); nm[..., 2] = rng.integers(150, 256, (8, 8))
    fs.textures = [nm]
    smooth = cs._quad(0.0, 1.0)
    n = np.asarray([[-0.3, 1.0, 0.2], [0.3, 1.0, 0.2], [0.3, 1.0, -0.2], [-0.3, 1.0, -0.2]], np.float64)
    smooth.normals = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    smooth.normal_indices = smooth.indices.copy()
    fs.meshes = [cs._quad(0.0, 1.0), smooth]
    parts = dict(PARTS)
    if edit_items:
        del parts["on_y"]
        parts["off_y_3e-4"] = (0, (1.1, 0.1, -1.2), (1.0, 1.0, 1.0), (0.6, 0.0, 0.2), False, False, True, True)
        parts["extra"] = EXTRA
    ids = {name: 3 * (k + 1) for k, name in enumerate(list(PARTS) + ["extra"])}
    for name, part in parts.items():
        _item(fs, name, part, ids[name], turn, attach and name == "plain")
    fs.lights = [Light(pos=(1.0, 6.0, 3.0), intensity=70.0), Light(dir=(0.3, -1.0, -0.4), color=(0.6, 0.7, 1.0), intensity=0.5, light_type=0)]
    cs._cam(fs, eye=(0.0, 5.0, 6.0), direction=(0.0, -0.75, -1.0), fov=60.0)
    return fs
