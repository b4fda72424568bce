"""Rays aimed at what a per-mesh tree walk can get wrong (rustray_amd/csrc/rr_walk.h: blas_closest, blas_any, blas_closest_packet):
shared vertices and edges (bit-equal toi in several triangles, in several leaves), points a few float32 spacings off them, rays in a
mesh's plane and in the planes of node boxes, axis-parallel rays with either sign of zero, and grazing rays near edges.

Everything here is numpy, seeded and built in code; nothing needs a GPU or the oracle.  tests/test_aimed_rays.py proves on the CPU
that these inputs are what they claim to be (ties exist and cross leaves, the oracle's own padded tree loses none of these rays);
tests/test_gpu_mesh_walk.py then holds the device walks to the oracle's brute-force form on them, bit for bit.

Coordinates of the lattice, the cube and the fans are multiples of 1/16 and the directions aimed at their vertices have components
that are powers of two, origins are `target - k * d` with k a power of two: every product of the triangle test is exact, so a ray
aimed at a shared vertex is accepted by all the triangles around it with ONE toi (= k), whatever plane they lie in.

The grazing cells (G) are |n.d| x distance in mesh sizes.  Cells that the CPU envelope test rejected are listed in DROPPED_G_CELLS
 and are not generated: none so far.  DROPPED_STARTS names the one kind of ray that was left out as a whole because
the oracle's own tree loses it.
"""
from __future__ import annotations

import functools

import numpy as np

from rustray_amd.flat import FlatScene, Item, Light, Material, MeshData
from rustray_amd.scene import Scene, get_transformation, inverse_affine

F32 = np.float32
MESHES = ("lattice", "cube", "soup", "fans")
INSTANCES = ("identity", "turned", "small", "general")
FAMILIES = ("V", "E", "U", "P", "A", "G")
EXACT_MESHES = ("lattice", "cube", "fans")     # meshes whose coordinates make the triangle test exact
PAD_REL = 4.0e-6                               # Builder::pad / pad_box: leaf boxes are padded by this much of their coordinates
G_SINES = (1e-1, 1e-2, 1e-3)                   # |n.d| of unit vectors
G_DISTANCES = (2.0, 10.0, 100.0)               # origin to target, in mesh sizes
DROPPED_G_CELLS: tuple = ()                    # (sine, distance) cells the CPU envelope test rejected: none
G_PER_CELL = 192
# Starts ON a triangle's plane (t = (o - a).n == 0) that leave it on the side its normal points to (n.d > 0) are NOT generated: the
# reference's triangle test picks its branch by the sign of t alone, so with t == 0 it takes the one written for n.d < 0, and accepts
# the triangle MIRRORED through its first vertex -- anywhere in the plane, outside the triangle's box, where no tree walk looks (the
# oracle's own tree differs from its brute-force form on 232 of 256 such rays at the lattice).  DESIGN.md D12.  Starts on the plane
# that leave it on the other side (n.d < 0: "V:toi0", "P:leave") take the branch written for them and are generated.
DROPPED_STARTS = ("on a plane, leaving on the normal's side",)


# ---------------------------------------------------------------------------------------------------------------------------
# meshes
# ---------------------------------------------------------------------------------------------------------------------------
class AimedMesh:
    """positions (V, 3) float32, indices (T, 3) uint32, and per triangle the unit normal on the side the aimed rays come from: the
    triangle's own (b - a) x (c - a), so that an aimed ray has n.d < 0."""

    def __init__(self, name, positions, indices, tri_n):
        self.name = name
        self.positions = np.ascontiguousarray(positions, F32)
        self.indices = np.ascontiguousarray(indices, np.uint32)
        self.tri_n = np.asarray(tri_n, np.float64)
        q = self.positions.astype(np.float64)[self.indices.astype(np.int64)]
        assert (np.einsum("ij,ij->i", np.cross(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0]), self.tri_n) > 0).all(), name
        self.size = float((self.positions.max(0) - self.positions.min(0)).max())
        self.pad = PAD_REL * float(np.abs(self.positions).max())   # one leaf pad, in mesh units
        edges = {}
        for f, (a, b, c) in enumerate(self.indices.tolist()):
            for e in ((a, b), (b, c), (c, a)):
                edges.setdefault((min(e), max(e)), []).append(f)
        self.edges = edges                                   # (v0, v1) -> faces
        inc = {}
        for f, tri in enumerate(self.indices.tolist()):
            for v in tri:
                inc.setdefault(v, []).append(f)
        self.incident = inc                                  # vertex -> faces
        self.v_targets = []                                  # (vertex, approach normals, least number of tied triangles)

    def data(self) -> MeshData:
        return MeshData(positions=self.positions.copy(), indices=self.indices.copy())

    def normals_at(self, faces):
        """The distinct approach normals of `faces`, in face order."""
        out = []
        for f in faces:
            n = tuple(np.round(self.tri_n[f], 9) + 0.0)
            if n not in out:
                out.append(n)
        return [np.asarray(n) for n in out]


def _grid_faces(nu, nv, vid, flip=False):
    """Two triangles per quad of an nu x nv grid with alternating diagonals; vid(i, j) -> vertex index.  Winding: u x v, or
    v x u with `flip`."""
    tris = []
    for i in range(nu):
        for j in range(nv):
            v00, v10, v11, v01 = vid(i, j), vid(i + 1, j), vid(i + 1, j + 1), vid(i, j + 1)
            tris += [(v00, v10, v11), (v00, v11, v01)] if (i + j) % 2 == 0 else [(v00, v10, v01), (v10, v11, v01)]
    return [(a, c, b) for a, b, c in tris] if flip else tris


def lattice() -> AimedMesh:
    """9 x 9 quads of side 0.25 in the plane y = 0.5, x and z from -1: 162 triangles, interior vertices shared by 4 or 8."""
    n = 9
    p = np.asarray([[-1.0 + 0.25 * i, 0.5, -1.0 + 0.25 * j] for i in range(n + 1) for j in range(n + 1)], F32)
    tris = _grid_faces(n, n, lambda i, j: i * (n + 1) + j, flip=True)   # x along i, z along j: z x x = +y
    m = AimedMesh("lattice", p, tris, np.tile([0.0, 1.0, 0.0], (len(tris), 1)))
    boundary = {v for e, fs in m.edges.items() if len(fs) == 1 for v in e}
    m.v_targets = [(v, m.normals_at(m.incident[v]), 4) for v in sorted(m.incident) if v not in boundary]
    assert len(tris) == 162 and len(m.v_targets) == 64
    return m


def cube() -> AimedMesh:
    """A closed axis-aligned cube of side 1.5, each face 3 x 3 quads: 108 triangles whose planes are planes of node boxes."""
    c = (-0.75, -0.25, 0.25, 0.75)
    verts, tris, normals = {}, [], []

    def vid(p):
        return verts.setdefault(tuple(p), len(verts))
    for a in range(3):
        for side in (-1.0, 1.0):
            u, v = (a + 1) % 3, (a + 2) % 3

            def at(i, j, a=a, side=side, u=u, v=v):
                p = [0.0, 0.0, 0.0]; p[a], p[u], p[v] = 0.75 * side, c[i], c[j]
                return vid(p)
            t = _grid_faces(3, 3, at, flip=side < 0)
            tris += t
            nrm = [0.0, 0.0, 0.0]; nrm[a] = side
            normals += [nrm] * len(t)
    p = np.asarray(sorted(verts, key=verts.get), F32)
    m = AimedMesh("cube", p, tris, normals)
    assert len(tris) == 108 and len(p) == 56 and all(len(fs) == 2 for fs in m.edges.values())
    for v in sorted(m.incident):
        ns = m.normals_at(m.incident[v])
        m.v_targets.append((v, ns, 2 if len(ns) == 3 else 4))   # corners: one or two triangles of each of three faces
    return m


def soup(seed=7) -> AimedMesh:
    """200 seeded random triangles in [-1, 1]^3, 20 of them slivers (a third vertex within 1e-3 of the opposite edge)."""
    rng = np.random.default_rng(seed)
    n, n_sliver = 200, 20
    c = rng.uniform(-0.85, 0.85, (n, 1, 3))
    p = c + rng.uniform(-0.15, 0.15, (n, 3, 3))
    for k in range(n_sliver):
        a, b = p[k, 0], p[k, 0] + rng.uniform(-0.3, 0.3, 3)
        p[k, 1] = b
        p[k, 2] = a + rng.uniform(0.2, 0.8) * (b - a) + rng.uniform(-1e-3, 1e-3, 3)
    p = p.astype(F32)
    q = p.astype(np.float64)
    nrm = np.cross(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return AimedMesh("soup", p.reshape(-1, 3), np.arange(3 * n).reshape(n, 3), nrm)


_RING = np.asarray([(2, 0), (2, 2), (0, 2), (-2, 2), (-2, 0), (-2, -2), (0, -2), (2, -2)], np.float64) * 0.25


def fan(n_tris) -> AimedMesh:
    """n_tris triangles (hub, r_k, r_k+3) around one hub in the plane y = 0.25, the r_k on a square ring.  The triangles overlap, so
    that no split pays for the builder and the whole mesh is ONE leaf (the root is a leaf code); every cross product of two ring
    vectors is a power of two, so all of them report one toi."""
    p = [(0.0, 0.25, 0.0)] + [(x, 0.25, z) for x, z in _RING]
    tris = [(0, 1 + (k + 3) % 8, 1 + k) for k in range(n_tris)]
    m = AimedMesh(f"fan{n_tris}", np.asarray(p, F32), tris, np.tile([0.0, 1.0, 0.0], (n_tris, 1)))
    m.v_targets = [(0, m.normals_at(m.incident[0]), 4)]
    return m


@functools.lru_cache(maxsize=None)
def mesh_parts(name):
    """name -> ((AimedMesh, offset in the scene's own frame), ...): one item per part."""
    if name == "lattice":
        return ((lattice(), (0.0, 0.0, 0.0)),)
    if name == "cube":
        return ((cube(), (0.0, 0.0, 0.0)),)
    if name == "soup":
        return ((soup(), (0.0, 0.0, 0.0)),)
    if name == "fans":   # both fans in ONE scene: lanes of one wave hold different one-leaf meshes
        return ((fan(8), (-1.0, 0.0, 0.0)), (fan(5), (1.0, 0.0, 0.0)))
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------------------------------------
# instances
# ---------------------------------------------------------------------------------------------------------------------------
class Instance:
    """x_world = M x + t.  `exact`: M is a signed permutation times a power of two and t is representable, so that rays and ties
    stay exact; `scale`: that power of two (directions are not scaled: a world ray keeps its length)."""

    def __init__(self, name, M, t, exact, scale=1.0):
        self.name, self.M, self.t, self.exact, self.scale = name, np.asarray(M, np.float64), np.asarray(t, np.float64), exact, scale

    def point(self, p):
        return np.asarray(p, np.float64) @ self.M.T + self.t

    def direction(self, d):
        return np.asarray(d, np.float64) @ (self.M / self.scale).T

    def matrix(self, offset):
        m = np.eye(4)
        m[:3, :3] = self.M
        m[:3, 3] = self.M @ np.asarray(offset, np.float64) + self.t
        return m


@functools.lru_cache(maxsize=None)
def instance(name) -> Instance:
    if name == "identity":
        return Instance(name, np.eye(3), (0.0, 0.0, 0.0), True)
    if name == "turned":      # a quarter turn about y and a representable translation
        return Instance(name, [[0, 0, 1], [0, 1, 0], [-1, 0, 0]], (2.0, -0.5, 1.0), True)
    if name == "small":       # 2^-10: a ray that starts 2 units away starts 1000 mesh sizes away in the mesh's own space
        return Instance(name, np.eye(3) * 2.0 ** -10, (0.0, 0.0, 0.0), True, 2.0 ** -10)
    if name == "general":     # parity only: ties are not promised
        m = get_transformation(np.eye(4, dtype=F32), (0.4, -0.3, 0.2), (1.3, 0.7, 1.1), (0.3, 0.4, 0.5)).astype(np.float64)
        return Instance(name, m[:3, :3], m[:3, 3], False)
    raise KeyError(name)


def scene(mesh_name, instance_name) -> FlatScene:
    """One item per part of the mesh, under the instance's transform."""
    inst = instance(instance_name)
    fs = FlatScene()
    for k, (m, off) in enumerate(mesh_parts(mesh_name)):
        fs.meshes.append(m.data())
        mat = Material(base_color=(0.7, 0.7, 0.7))
        fs.materials.append(mat); fs.materials.append(Scene._cache_of(mat))
        t = inst.matrix(off).astype(F32)
        ti = inverse_affine(t)
        if inst.exact:
            assert (t.astype(np.float64) == inst.matrix(off)).all()
            assert (ti.astype(np.float64) @ t.astype(np.float64) == np.eye(4)).all(), (mesh_name, instance_name)
        fs.items.append(Item(kind=1, id=3 + k, material=2 * k, material_cache=2 * k + 1, mesh=k, trans=t, trans_inv=ti,
                             bbox_min=tuple(m.positions.min(0)), bbox_max=tuple(m.positions.max(0)), name=m.name))
    lo = np.min([inst.point(m.positions.astype(np.float64) + off).min(0) for m, off in mesh_parts(mesh_name)], 0)
    hi = np.max([inst.point(m.positions.astype(np.float64) + off).max(0) for m, off in mesh_parts(mesh_name)], 0)
    fs.lights = [Light(pos=tuple((0.5 * (lo + hi) + (0.0, 3.0 * (hi - lo).max(), 0.0)).tolist()), intensity=10.0)]
    fs.meta = {"camera": dict(width=64, height=64, fov=1.0, eye_pos=(0.5 * (lo + hi) + (0.0, 0.0, 3.0 * (hi - lo).max())).tolist(),
                              up=[0.0, 1.0, 0.0], dir=[0.0, 0.0, -1.0], clipping_near=0.1, clipping_far=1000.0)}
    return fs


# ---------------------------------------------------------------------------------------------------------------------------
# ray families
# ---------------------------------------------------------------------------------------------------------------------------
class Rays:
    """origins, directions (n, 3) float32; per ray: label ("V:diag" ...), item and face it is aimed at (-1: none), the least
    number of triangles that must tie at one toi (0: no claim), the exact number (0: no claim) and whether it must miss."""

    def __init__(self):
        self.o, self.d, self.label, self.item, self.face, self.min_ties, self.n_ties, self.must_miss = [], [], [], [], [], [], [], []

    def add(self, o, d, label, item=-1, face=-1, min_ties=0, n_ties=0, must_miss=False, exact=False):
        o64, d64 = np.asarray(o, np.float64), np.asarray(d, np.float64)
        o32, d32 = o64.astype(F32), d64.astype(F32)
        if exact:
            assert (o32.astype(np.float64) == o64).all() and (d32.astype(np.float64) == d64).all(), (label, o64, d64)
        self.o.append(o32); self.d.append(d32); self.label.append(label); self.item.append(item); self.face.append(face)
        self.min_ties.append(min_ties); self.n_ties.append(n_ties); self.must_miss.append(must_miss)

    def done(self):
        self.o = np.asarray(self.o, F32).reshape(-1, 3); self.d = np.asarray(self.d, F32).reshape(-1, 3)
        self.label = np.asarray(self.label); self.item = np.asarray(self.item, np.int64); self.face = np.asarray(self.face, np.int64)
        self.min_ties = np.asarray(self.min_ties, np.int64); self.n_ties = np.asarray(self.n_ties, np.int64)
        self.must_miss = np.asarray(self.must_miss, bool)
        return self

    def __len__(self):
        return len(self.o)

    def take(self, idx):
        r = Rays()
        for k in ("o", "d", "label", "item", "face", "min_ties", "n_ties", "must_miss"):
            setattr(r, k, getattr(self, k)[idx])
        return r

    def sorted_order(self, lanes=64):
        """Coherent waves: by direction octant, label, item and target triangle; directions with a zero component (they never form
        a packet) last.  Every octant's run is filled up to a multiple of `lanes` by repeating its last ray (as the kernels fill
        the last packet of a batch), so that no wave mixes two octants: an index array with repeats, every ray at least once."""
        zero = (self.d == 0).any(axis=1)
        octant = np.where(zero, 8, np.signbit(self.d) @ np.asarray([1, 2, 4]))
        _, lab = np.unique(self.label, return_inverse=True)
        order = np.lexsort((self.face, self.item, lab, octant))
        out = []
        for k in np.unique(octant):
            run = order[octant[order] == k]
            out.append(np.concatenate([run, np.repeat(run[-1:], -len(run) % lanes)]))
        return np.concatenate(out)

    def permuted_order(self, seed=5):
        return np.random.default_rng(seed).permutation(len(self))


def _signs(normals):
    """+-1 per axis: the side the rays come from (the sum of the approach normals; +1 where that is zero)."""
    s = np.sum(normals, axis=0)
    return np.where(s != 0, np.sign(s), 1.0)


def _generic(n, along):
    """Directions at a surface whose coordinates are not special (the soup): straight down the normal, and tilted along `along`."""
    return {"axis": -n, "diag": -n + 0.5 * along, "gen": -n - 0.3 * along + 0.2 * np.cross(n, along)}


def _aimed_dirs(mesh_name, normals, along=None):
    """name -> direction (own frame) for rays aimed at a point with these approach normals.  Exact meshes: components that are powers
    of two."""
    if mesh_name not in EXACT_MESHES:
        return _generic(normals[0], along)
    s = _signs(normals)
    out = {"diag": -s * np.asarray([1.0, 1.0, 1.0])}
    a = int(np.argmax(np.abs(normals[0])))
    g = np.asarray([0.5, 0.5, 0.5]); g[a] = 1.0; g[(a + 2) % 3] = 0.25
    out["gen"] = -s * g
    if len(normals) == 1:
        out["axis"] = -normals[0] + 0.0
    return out


def _edge_targets(m: AimedMesh, rng, n_shared=None):
    """(point, faces, approach normals, unit edge direction) at 1/2 and 1/4 of every boundary edge and of shared edges (all of them,
    or a seeded choice of n_shared)."""
    q = m.positions.astype(np.float64)
    shared = sorted(e for e, fs in m.edges.items() if len(fs) == 2)
    boundary = sorted(e for e, fs in m.edges.items() if len(fs) == 1)
    if n_shared is not None and len(shared) > n_shared:
        shared = [shared[i] for i in sorted(rng.choice(len(shared), n_shared, replace=False))]
    out = []
    for e in shared + boundary:
        a, b = q[e[0]], q[e[1]]
        for f in (0.5, 0.25):
            out.append((a + f * (b - a), m.edges[e], m.normals_at(m.edges[e]), (b - a) / np.linalg.norm(b - a)))
    return out


def _family_V(R, mesh_name, inst, part, m, off):
    q = m.positions.astype(np.float64) + off
    for v, normals, least in m.v_targets:
        P = inst.point(q[v])
        face = m.incident[v][0]
        least = least if inst.exact else 0
        dirs = _aimed_dirs(mesh_name, normals)
        for name, k in (("axis", 2.0), ("diag", 2.0), ("gen", 4.0)):
            if name not in dirs:
                continue
            d = inst.direction(dirs[name])
            R.add(P - k * d, d, f"V:{name}", part, face, least, exact=inst.exact)
        zero = "axis" if "axis" in dirs else "diag"
        R.add(P, inst.direction(dirs[zero]), "V:toi0", part, face, least, exact=inst.exact)   # the origin ON the vertex
        if len(normals) == 1:   # from the other side, with -0.0 in the idle components
            d = inst.direction(normals[0])
            d = np.where(d == 0, -0.0, d)
            R.add(P - 2.0 * d, d, "V:back", part, face, least, exact=inst.exact)


def _family_E(R, mesh_name, inst, part, m, off, rng):
    exact_mesh = mesh_name in EXACT_MESHES
    for i, (p, faces, normals, along) in enumerate(_edge_targets(m, rng, 120 if mesh_name != "soup" else None)):
        P = inst.point(p + off)
        dirs = _aimed_dirs(mesh_name, normals, along)
        names = [n for n in ("axis", "diag", "gen") if n in dirs]
        name = names[i % len(names)]
        d = inst.direction(dirs[name])
        exact = inst.exact and exact_mesh
        # a fan's triangles overlap (see fan()): a point of a shared edge lies in others too, so the exact count is lattice and cube only
        n_ties = 2 if exact and len(faces) == 2 and not m.name.startswith("fan") else 0
        R.add(P - 2.0 * d, d, f"E:{name}", part, faces[0], 2 if exact and len(faces) == 2 else 0, n_ties, exact=exact)


def _in_plane_axes(mesh_name, normal, along):
    if mesh_name in EXACT_MESHES:
        a = int(np.argmax(np.abs(normal)))
        e = np.eye(3)
        return e[(a + 1) % 3], e[(a + 2) % 3]
    return along, np.cross(normal, along)


def _family_U(R, mesh_name, inst, part, m, off, rng):
    """The V and E targets moved by +-1 and +-4 float32 spacings (of the world coordinate) along each in-plane axis.  The direction's
    component along the moved axis is 2^-5 towards zero, so that the origin keeps the moved coordinate's spacing and the move survives
    the rounding of the origin (exact instances); no component is zero, so the rays can form packets."""
    q = m.positions.astype(np.float64) + off
    targets = [(q[v], m.incident[v][0], normals[0], None) for v, normals, _ in m.v_targets]
    targets += [(p + off, faces[0], normals[0], along) for p, faces, normals, along in _edge_targets(m, rng, 60 if mesh_name != "soup" else None)]
    Mn = inst.M / np.linalg.norm(inst.M, axis=0, keepdims=True)
    for i, (p, face, normal, along) in enumerate(targets):
        P = inst.point(p)
        n_w = Mn @ normal
        axes = _in_plane_axes(mesh_name, normal, along)
        for a in range(2):
            u, w = Mn @ axes[a], Mn @ axes[1 - a]
            j = int(np.argmax(np.abs(u)))
            sp = float(np.spacing(F32(abs(P[j]))))
            towards = 1.0 if P @ u >= 0 else -1.0
            d = -n_w + towards * 2.0 ** -5 * inst.scale * u + (0.25 if (i + a) % 2 else -0.25) * w
            for step in (-4, -1, 1, 4):
                moved = P + step * sp * u
                R.add(moved - 2.0 * d, d, "U", part, face)


def _family_P(R, mesh_name, inst, part, m, off, rng):
    """Rays IN a mesh plane along lattice lines (every triangle of that plane has d.n == 0: a planar mesh must miss), and rays that
    start on the plane, at a vertex and inside a triangle, and leave it against the normal, straight and tilted (DROPPED_STARTS has
    the other side)."""
    if mesh_name not in EXACT_MESHES:
        return
    q = m.positions.astype(np.float64) + off
    lo, hi = q.min(0), q.max(0)
    planar = len({tuple(n) for n in np.round(m.tri_n, 9)}) == 1
    seen = set()
    for f, tri in enumerate(m.indices.tolist()):
        n = m.tri_n[f]
        a = int(np.argmax(np.abs(n)))
        for v in tri:
            for b in ((a + 1) % 3, (a + 2) % 3):      # the line through this vertex along axis b, in the plane of face f
                key = (a, float(q[v][a]), b, tuple(np.delete(q[v], b)))
                if key in seen:
                    continue
                seen.add(key)
                for sgn in (1.0, -1.0):
                    start = q[v].copy(); start[b] = (lo[b] - 0.5) if sgn > 0 else (hi[b] + 0.5)
                    d = np.zeros(3); d[b] = sgn
                    d = np.where(d == 0, -0.0 if sgn < 0 else 0.0, d)
                    R.add(inst.point(start), inst.direction(d), "P:in", part, f, must_miss=planar and inst.exact, exact=inst.exact)
    for i, (v, normals, _) in enumerate(m.v_targets):
        if len(normals) != 1:      # (on a crease the tilted ray would leave the OTHER face on its outer side: see DROPPED_STARTS)
            continue
        n = normals[0]
        a = int(np.argmax(np.abs(n)))
        tilt = np.zeros(3); tilt[(a + 1) % 3], tilt[(a + 2) % 3] = 0.5, -0.25
        centre = np.asarray([0.5, 0.25, 0.25]) @ q[m.indices[m.incident[v][0]]]   # a point inside the first triangle at v
        for start in (q[v], centre):
            for t in (0.0, 1.0):
                R.add(inst.point(start), inst.direction(-n + t * tilt), "P:leave", part, m.incident[v][0], exact=inst.exact)


def _family_A(R, mesh_name, inst):
    """Axis-parallel rays (own frame) on a grid of step 1/4 through the mesh's box and one step around it, lattice coordinates among
    the origins, either sign of zero in the idle components."""
    q = np.concatenate([m.positions.astype(np.float64) + off for m, off in mesh_parts(mesh_name)])
    lo, hi = np.floor(q.min(0) * 4.0) / 4.0 - 0.25, np.ceil(q.max(0) * 4.0) / 4.0 + 0.25
    g = [np.arange(round((hi[a] - lo[a]) * 4.0) + 1) / 4.0 + lo[a] for a in range(3)]
    i = 0
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        for sgn in (1.0, -1.0):
            for x in g[b]:
                for y in g[c]:
                    o = np.zeros(3); o[a], o[b], o[c] = (lo[a] - 1.0) if sgn > 0 else (hi[a] + 1.0), x, y
                    d = np.zeros(3); d[a] = sgn
                    dw = inst.direction(d)
                    dw = np.where(dw == 0, -0.0 if i % 2 else 0.0, dw)
                    R.add(inst.point(o), dw, "A", exact=inst.exact)
                    i += 1


def _family_G(R, mesh_name, inst, part, m, off, rng):
    """Grazing rays: per cell (|n.d|, distance in mesh sizes), G_PER_CELL rays aimed at points within +-40 leaf pads of an edge, on
    both sides of it; two thirds of the edges are hull edges where the mesh has any.  The whole ray is mapped into the world, so the
    distance is in mesh sizes of the mesh's own space under every instance."""
    if mesh_name not in ("lattice", "soup"):
        return
    q = m.positions.astype(np.float64) + off
    hull = sorted(e for e, fs in m.edges.items() if len(fs) == 1)
    inner = sorted(e for e, fs in m.edges.items() if len(fs) == 2) or hull
    for sine in G_SINES:
        for dist in G_DISTANCES:
            if (sine, dist) in DROPPED_G_CELLS:
                continue
            for k in range(G_PER_CELL):
                pool = hull if k % 3 else inner
                e = pool[int(rng.integers(0, len(pool)))]
                f = m.edges[e][int(rng.integers(0, len(m.edges[e])))]
                n = m.tri_n[f]
                a, b = q[e[0]], q[e[1]]
                along = (b - a) / np.linalg.norm(b - a)
                across = np.cross(n, along)
                aim = a + rng.uniform(0.05, 0.95) * (b - a) + rng.uniform(-40.0, 40.0) * m.pad * across
                phi = rng.uniform(0.0, 2.0 * np.pi)
                tangent = np.cos(phi) * along + np.sin(phi) * across
                d = np.sqrt(1.0 - sine * sine) * tangent + (sine if k % 2 else -sine) * n
                o = aim - dist * m.size * d
                ow, dw = inst.point(o), np.asarray(d) @ inst.M.T
                R.add(ow, dw / np.linalg.norm(dw) if not inst.exact else dw / inst.scale, f"G:{sine:g}:{dist:g}", part, f)


@functools.lru_cache(maxsize=None)
def rays(mesh_name, instance_name, family) -> Rays:
    """The rays of one family for one scene(mesh_name, instance_name), in generation order (use sorted_order / permuted_order)."""
    inst = instance(instance_name)
    R = Rays()
    rng = np.random.default_rng([MESHES.index(mesh_name), FAMILIES.index(family), 11])
    if family == "A":
        _family_A(R, mesh_name, inst)
        return R.done()
    for part, (m, off) in enumerate(mesh_parts(mesh_name)):
        off = np.asarray(off, np.float64)
        if family == "V":
            _family_V(R, mesh_name, inst, part, m, off)
        elif family == "E":
            _family_E(R, mesh_name, inst, part, m, off, rng)
        elif family == "U":
            _family_U(R, mesh_name, inst, part, m, off, rng)
        elif family == "P":
            _family_P(R, mesh_name, inst, part, m, off, rng)
        elif family == "G":
            _family_G(R, mesh_name, inst, part, m, off, rng)
        else:
            raise KeyError(family)
    return R.done()


def all_rays(mesh_name, instance_name, families=FAMILIES) -> Rays:
    """The families of one scene in one batch (families without rays for this mesh left out)."""
    parts = [rays(mesh_name, instance_name, f) for f in families]
    parts = [p for p in parts if len(p)]
    out = Rays()
    for k in ("o", "d", "label", "item", "face", "min_ties", "n_ties", "must_miss"):
        setattr(out, k, np.concatenate([getattr(p, k) for p in parts]))
    return out


def local_rays(fs: FlatScene, item: int, o, d):
    """The rays in the item's own space, as Shape::get_inverse_ray forms them, in float64 (exact for the exact instances)."""
    ti = np.asarray(fs.items[item].trans_inv, np.float64)
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    return o @ ti[:3, :3].T + ti[:3, 3], d @ ti[:3, :3].T
