"""Builders of the adversarial scenes of tests/test_gpu_corners.py, shared with tests/test_gpu_packet_walk.py (which traces the
same scenes through the packet form of the top level) and tests/test_packet_pad.py."""
import numpy as np

from rustray_amd.flat import FlatScene, Item, Light, Material, MeshData
from rustray_amd.scene import Scene

EYE = np.eye(4, dtype=np.float32)


def _mat(fs, m):
    fs.materials.append(m); fs.materials.append(Scene._cache_of(m))
    return len(fs.materials) - 2, len(fs.materials) - 1


def _quad(y, half, uv=True):
    p = np.asarray([[-half, y, half], [half, y, half], [half, y, -half], [-half, y, -half]], np.float32)
    md = MeshData(positions=p, indices=np.asarray([[0, 1, 2], [0, 2, 3]], np.uint32))
    if uv:
        md.uvs = np.asarray([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
        md.uv_indices = np.asarray([[0, 1, 2], [0, 2, 3]], np.uint32)
    return md


def _mesh_item(fs, mesh, mat, idn, name, bbox=None, trans=None, trans_inv=None):
    p = fs.meshes[mesh].positions
    mi, ci = _mat(fs, mat)
    lo, hi = (tuple(p.min(0)), tuple(p.max(0))) if bbox is None else bbox
    fs.items.append(Item(kind=1, id=idn, material=mi, material_cache=ci, mesh=mesh, trans=(EYE if trans is None else trans).copy(),
                         trans_inv=(EYE if trans_inv is None else trans_inv).copy(), bbox_min=lo, bbox_max=hi, name=name))


def _cam(fs, eye=(0.0, 6.0, 9.0), direction=(0.0, -0.6, -1.0), fov=60.0):
    fs.meta = {"camera": dict(width=64, height=64, fov=float(np.float32(np.radians(fov))), eye_pos=list(eye), up=[0.0, 1.0, 0.0],
                              dir=list(direction), clipping_near=0.1, clipping_far=100.0)}


def equal_toi_scene(thick=False):
    """Two items share ONE mesh (bit-equal toi): red (id 3, index 0) and green (id 6, index 1).  `thick`: green's declared box
    is thicker, so it is entered earlier."""
    fs = FlatScene()
    fs.meshes = [_quad(0.0, 5.0)]
    _mesh_item(fs, 0, Material(base_color=(1.0, 0.1, 0.1)), 3, "red")
    _mesh_item(fs, 0, Material(base_color=(0.1, 1.0, 0.1)), 6, "green")
    fs.lights = [Light(pos=(0.0, 8.0, 0.0), intensity=80.0)]
    _cam(fs)
    if thick:
        fs.items[1].bbox_min, fs.items[1].bbox_max = (-5.0, -1.0, -5.0), (5.0, 1.0, 5.0)
    return fs


def alpha_occluder_scene(nearest=False):
    """An alpha-mapped, semi-transparent occluder over a textured floor; its second face has no uv indices."""
    fs = FlatScene()
    rng = np.random.default_rng(4)
    alpha = np.zeros((16, 16, 4), np.uint8); alpha[..., :3] = (rng.integers(0, 2, (16, 16, 1)) * 255).astype(np.uint8); alpha[..., 3] = 255
    base = np.full((8, 8, 4), 255, np.uint8); base[::2, ::2, :3] = 60
    fs.textures = [alpha, base]
    floor, cover = _quad(0.0, 10.0), _quad(3.0, 2.5)
    cover.uv_indices = cover.uv_indices[:1]                                  # second face has no uv indices -> uv (0,0)
    fs.meshes = [floor, cover]
    fm = Material(base_color=(0.9, 0.9, 0.9)); fm.texture[0] = 1
    _mesh_item(fs, 0, fm, 3, "floor")
    cm = Material(base_color=(0.2, 0.3, 0.9), alpha=0.7, refraction_index=1.2); cm.texture[4] = 0; cm.texture[0] = 1
    _mesh_item(fs, 1, cm, 6, "cover")
    fs.lights = [Light(pos=(1.0, 9.0, 2.0), intensity=90.0), Light(pos=(-3.0, 6.0, -1.0), color=(1.0, 0.6, 0.3), intensity=50.0)]
    _cam(fs)
    fs.materials[fs.items[1].material].texture_filtering_nearest = nearest
    return fs


def inside_spheres_scene(alpha, cull):
    """The camera inside a ball of radius 6 (solid or not), a second ball in front of it."""
    fs = FlatScene()
    m = Material(base_color=(0.7, 0.8, 0.9), alpha=alpha, backface_cullig=cull, reflectivity=0.2, refraction_index=1.3)
    mi, ci = _mat(fs, m)
    fs.items = [Item(kind=0, id=3, material=mi, material_cache=ci, radius=6.0, bbox_min=(-6.0,) * 3, bbox_max=(6.0,) * 3, name="shell")]
    m2 = Material(base_color=(0.9, 0.4, 0.1))
    mi2, ci2 = _mat(fs, m2)
    t = EYE.copy(); t[:3, 3] = (0.5, -0.5, -3.0); ti = EYE.copy(); ti[:3, 3] = (-0.5, 0.5, 3.0)
    fs.items.append(Item(kind=0, id=6, material=mi2, material_cache=ci2, radius=1.0, trans=t, trans_inv=ti, bbox_min=(-1.0,) * 3, bbox_max=(1.0,) * 3, name="ball"))
    fs.lights = [Light(pos=(1.0, 2.0, 1.0), intensity=30.0)]
    _cam(fs, eye=(0.0, 0.0, 0.0), direction=(0.0, 0.0, -1.0), fov=80.0)
    return fs


INSIDE_SPHERES = ((1.0, True), (1.0, False), (0.6, True))


def projective_scene():
    """A ball whose inverse has the w row (0, 0, 0, 2) (compensated in the first three rows), over a reflective floor."""
    fs = FlatScene()
    fs.meshes = [_quad(0.0, 4.0)]
    _mesh_item(fs, 0, Material(base_color=(0.8, 0.8, 0.8), reflectivity=0.3), 3, "floor")
    s = np.diag(np.asarray([1.5, 0.6, 1.0, 1.0], np.float32)); s[:3, 3] = (0.0, 1.5, -1.0)
    si = np.linalg.inv(s.astype(np.float64)).astype(np.float32)
    si[3, :] = (0.0, 0.0, 0.0, 2.0)                                          # homogeneous scale: origin' = (M x) / 2
    si[:3, :] *= 2.0                                                        # ... compensated in the first three rows
    m = Material(base_color=(0.2, 0.7, 0.3), alpha=0.5, refraction_index=1.4, reflectivity=0.3)
    mi, ci = _mat(fs, m)
    fs.items.append(Item(kind=0, id=6, material=mi, material_cache=ci, radius=1.0, trans=s, trans_inv=si, bbox_min=(-1.0,) * 3, bbox_max=(1.0,) * 3, name="ellipsoid"))
    fs.lights = [Light(pos=(2.0, 7.0, 3.0), intensity=70.0)]
    _cam(fs, eye=(0.0, 3.0, 6.0), direction=(0.0, -0.35, -1.0))
    return fs


def deep_mesh_scene():
    """A geometric progression of nested triangles (a per-mesh tree at the builder's depth limit) over a floor."""
    n = 600
    s = (4.0 * 0.97 ** np.arange(n)).astype(np.float32)
    z = (-0.004 * np.arange(n)).astype(np.float32)
    p = np.zeros((n, 3, 3), np.float32)
    p[:, 1, 0] = s; p[:, 2, 1] = s
    p[:, :, 2] = z[:, None]
    p[:, :, :2] -= 1.0
    fs = FlatScene()
    fs.meshes = [MeshData(positions=p.reshape(-1, 3), indices=np.arange(3 * n, dtype=np.uint32).reshape(n, 3)), _quad(-1.5, 6.0, uv=False)]
    _mesh_item(fs, 0, Material(base_color=(0.9, 0.6, 0.2), reflectivity=0.2), 2, "fan")
    _mesh_item(fs, 1, Material(base_color=(0.5, 0.5, 0.6)), 4, "floor")
    fs.lights = [Light(pos=(2.0, 3.0, 5.0), intensity=60.0)]
    _cam(fs, eye=(0.5, 0.8, 5.0), direction=(-0.1, -0.15, -1.0))
    return fs


def zero_light_term_scene(degenerate):
    """A light below the floor (every light term exactly zero) and an alpha-mapped occluder below it; the floor's third face is
    degenerate (its uv can be NaN) or a proper sliver."""
    rng = np.random.default_rng(9)
    alpha = np.zeros((8, 8, 4), np.uint8); alpha[..., :3] = rng.integers(40, 255, (8, 8, 1)).astype(np.uint8); alpha[..., 3] = 255
    fs = FlatScene()
    fs.textures = [alpha]
    floor = _quad(0.0, 6.0)
    # a third face: degenerate (three collinear vertices) or a proper sliver beside the quad
    third = [[7.0, 0.0, 0.0], [8.0, 0.0, 0.0], [9.0, 0.0, 0.0]] if degenerate else [[7.0, 0.0, 0.0], [8.0, 0.0, 0.0], [8.0, 0.0, -1.0]]
    floor.positions = np.concatenate([floor.positions, np.asarray(third, np.float32)])
    floor.indices = np.concatenate([floor.indices, np.asarray([[4, 5, 6]], np.uint32)])
    floor.uvs = np.concatenate([floor.uvs, np.asarray([[0.2, 0.2], [0.8, 0.3], [0.5, 0.9]], np.float32)])
    floor.uv_indices = np.concatenate([floor.uv_indices, np.asarray([[4, 5, 6]], np.uint32)])
    # the occluder BELOW the floor, three faces so that face id 2 exists: the receiver's face 2 is the third one
    p = np.asarray([[-4, -2, 4], [4, -2, 4], [4, -2, -4], [-4, -2, -4], [0, -2, 0]], np.float32)
    cover = MeshData(positions=p, indices=np.asarray([[0, 1, 4], [1, 2, 4], [2, 3, 0]], np.uint32),
                     uvs=np.asarray([[0, 0], [1, 0], [1, 1], [0, 1], [0.5, 0.5]], np.float32), uv_indices=np.asarray([[0, 1, 4], [1, 2, 4], [2, 3, 0]], np.uint32))
    fs.meshes = [floor, cover]
    fm = Material(base_color=(0.6, 0.6, 0.6), specular_color=(0.0, 0.0, 0.0), ambient_color=(0.2, 0.1, 0.05), cast_shadow=False)
    _mesh_item(fs, 0, fm, 3, "floor")
    cm = Material(base_color=(0.3, 0.3, 0.9)); cm.texture[4] = 0     # alpha map, bilinear (the default filter)
    _mesh_item(fs, 1, cm, 6, "cover")
    fs.lights = [Light(pos=(0.5, -9.0, -0.5), intensity=60.0)]        # BELOW the floor: dot(normal, to_light) < 0, the term is exactly zero
    _cam(fs)
    return fs


def blocker_scene():
    """tests/test_gpu_parity.py::_blocker_scene: a sphere behind a point light precedes, in bbox-distance order, an occluder
    whose box reaches past the light."""
    from tests.test_gpu_parity import _blocker_scene
    return _blocker_scene()


def builders():
    """name -> builder of every scene above (the corner scenes in each of their variants)."""
    out = {"equal_toi": equal_toi_scene, "equal_toi_thick": lambda: equal_toi_scene(True),
           "alpha_occluder": alpha_occluder_scene, "alpha_occluder_nearest": lambda: alpha_occluder_scene(True),
           "projective": projective_scene, "deep_mesh": deep_mesh_scene,
           "zero_term_degenerate": lambda: zero_light_term_scene(True), "zero_term_sliver": lambda: zero_light_term_scene(False),
           "blocker": blocker_scene}
    for a, c in INSIDE_SPHERES:
        out[f"inside_spheres_{a}_{int(c)}"] = (lambda a=a, c=c: inside_spheres_scene(a, c))
    return out
