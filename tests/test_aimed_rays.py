"""tests/aimed_rays.py gives the GPU tests (tests/test_gpu_mesh_walk.py) what they need: shown here on the CPU, as conditions.

* Ties exist and cross leaves: every ray aimed at a shared vertex is accepted by several triangles with ONE bit-equal toi (the
  oracle's single-triangle test, rro_ray_triangle), every ray at a shared edge by exactly two; the tied faces of the lattice fall in
  at least two leaves of the tree rr_bvh.cpp builds (tests/native/mesh_leaves.cpp), whose leaves hold 1, 5 and 8 triangles somewhere.
* The brute-force winner of a tie is the lowest tied face.
* The envelope: the oracle's own padded tree (the pad of Builder::pad, exact reciprocals) loses none of these rays; no ray is excused.
* Effectiveness: U and G have at least a quarter hits and a quarter misses.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import aimed_rays as ar
from tests.helpers import ROOT

CASES = [(m, i) for m in ar.MESHES for i in ar.INSTANCES]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def accepting(oracle, mesh, o, d):
    """{face: toi bits} of the triangles of `mesh` that accept the own-space ray (o, d)."""
    o, d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
    P = mesh.positions
    toi, n, back = C.c_float(0), np.zeros(3, np.float32), C.c_int(0)
    f = oracle.lib().rro_ray_triangle
    out = {}
    for face, (a, b, c) in enumerate(mesh.indices):
        if f(_p(P[a]), _p(P[b]), _p(P[c]), _p(o), _p(d), C.byref(toi), _p(n), C.byref(back)):
            out[face] = np.float32(toi.value).view(np.uint32).item()
    return out


@functools.lru_cache(maxsize=None)
def _brute(oracle, mesh_name, inst_name, family):
    R = ar.rays(mesh_name, inst_name, family)
    fs = ar.scene(mesh_name, inst_name)    # (the struct borrows the scene's buffers: the scene stays alive over the call)
    return oracle.trace_rays(fs.c_struct(), R.o, R.d, 1, brute_force=True)


def _own_space(fs, item, o, d):
    lo, ld = ar.local_rays(fs, item, o, d)
    o32, d32 = lo.astype(np.float32), ld.astype(np.float32)
    assert (o32 == lo).all() and (d32 == ld).all()          # exact instances: the own-space ray is exact
    return o32, d32


@pytest.mark.parametrize("mesh_name", ar.EXACT_MESHES)
@pytest.mark.parametrize("inst_name", [i for i in ar.INSTANCES if ar.instance(i).exact])
def test_aimed_rays_tie_and_the_lowest_face_wins(oracle, mesh_name, inst_name):
    """V: at least 4 triangles (2 at a cube corner) accept the ray with one bit-equal toi; E on a shared edge: exactly 2 (lattice,
    cube), at least 2 (the fans' overlapping triangles).  The brute-force winner is the lowest face among those of the smallest toi."""
    fs = ar.scene(mesh_name, inst_name)
    parts = ar.mesh_parts(mesh_name)
    n_v = n_e = n_first = 0
    for family in ("V", "E"):
        R = ar.rays(mesh_name, inst_name, family)
        found, item, face, toi = _brute(oracle, mesh_name, inst_name, family)
        claimed = np.flatnonzero((R.min_ties > 0) | (R.n_ties > 0))
        assert len(claimed) > 0 and (family == "E" or len(claimed) == len(R))
        for i in claimed:
            mesh = parts[R.item[i]][0]
            acc = accepting(oracle, mesh, *_own_space(fs, int(R.item[i]), R.o[i], R.d[i]))
            by_toi = {}
            for f, bits in acc.items():
                by_toi.setdefault(bits & 0x7fffffff if bits == 0x80000000 else bits, []).append(f)   # (-0.0 ties with 0.0: toi == best)
            ties = next((g for g in by_toi.values() if int(R.face[i]) in g), [])   # the tie at the point the ray is aimed at
            what = (mesh_name, inst_name, R.label[i], int(i), acc)
            assert len(ties) >= R.min_ties[i], what
            if R.n_ties[i]:
                assert len(ties) == R.n_ties[i], what              # (a ray through the closed cube leaves it through other triangles, later)
            # the winner: of the faces with the smallest toi (non-negative floats order as their bits) the lowest
            first = min(by_toi)
            assert found[i], what
            if item[i] == R.item[i]:
                assert face[i] % len(mesh.indices) == min(by_toi[first]) and toi[i].view(np.uint32) == acc[min(by_toi[first])], what
                n_first += len(by_toi[first]) >= 2
            n_v += family == "V"; n_e += family == "E"
    assert n_v > 0 and n_e > 0 and n_first >= (n_v + n_e) // 2   # most of the ties are ties of the CLOSEST hit


@pytest.fixture(scope="module")
def leaf_tool(tmp_path_factory):
    """m -> [(parent node, [faces])]: the leaves of the tree the device walks for an AimedMesh (tests/native/mesh_leaves.cpp)."""
    exe = str(tmp_path_factory.mktemp("mesh_leaves") / "mesh_leaves")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "mesh_leaves.cpp"), os.path.join(ROOT, "rustray_amd", "csrc", "rr_bvh.cpp")])
    return lambda m: _leaves_of(exe, m)


def _leaves_of(exe, m):
    tri = m.positions[m.indices.astype(np.int64)]
    lo, hi = tri.min(axis=1), tri.max(axis=1)
    text = f"{len(lo)}\n" + "".join(" ".join(f"{v:.9g}" for v in np.concatenate([a, b])) + "\n" for a, b in zip(lo, hi))
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    res = []
    for line in out.stdout.splitlines():
        w = line.split()
        if w[0] == "leaf":
            assert int(w[2]) == len(w) - 3
            res.append((int(w[1]), [int(x) for x in w[3:]]))
    assert sorted(f for _, fs in res for f in fs) == list(range(len(m.indices)))
    return res


def test_tied_faces_fall_in_several_leaves_and_leaf_sizes_1_5_8_occur(oracle, leaf_tool):
    """The tree of rr_bvh.cpp for these meshes: each fan is ONE leaf (the root is a leaf code) of 8 and of 5 triangles, some leaf is a
    singleton, and the faces that tie at an interior lattice vertex lie in two lattice rows and in at least two leaves, at every one
    of the 64 vertices (a walk that keeps the first of the tied faces it meets, or prunes a leaf at equality, changes these rays)."""
    tool = leaf_tool
    counts = set()
    for name in ar.MESHES:
        for m, _ in ar.mesh_parts(name):
            lv = tool(m)
            counts |= {len(fs) for _, fs in lv}
            if m.name.startswith("fan"):
                assert lv == [(-1, list(range(len(m.indices))))] or (len(lv) == 1 and lv[0][0] == -1), (m.name, lv)
    assert {1, 5, 8} <= counts, counts
    m = ar.mesh_parts("lattice")[0][0]
    lv = tool(m)
    assert len(lv) >= 16 and len({p for p, _ in lv}) >= 4          # several BVH4 nodes hold the leaves
    leaf_of = {f: k for k, (_, fs) in enumerate(lv) for f in fs}
    row_of = lambda f: f // 18                                      # 9 quads of two triangles per lattice row
    fs = ar.scene("lattice", "identity")
    R = ar.rays("lattice", "identity", "V")
    split = rows = 0
    sel = np.flatnonzero(R.label == "V:diag")
    for i in sel:
        acc = accepting(oracle, m, *_own_space(fs, 0, R.o[i], R.d[i]))
        assert len(acc) >= 4 and len(set(acc.values())) == 1    # one bit-equal toi
        split += len({leaf_of[f] for f in acc}) >= 2
        rows += len({row_of(f) for f in acc}) >= 2
    assert rows == len(sel) == 64          # the triangles around an interior vertex lie in two lattice rows
    assert split == len(sel), (split, len(sel))


@pytest.mark.parametrize("mesh_name,inst_name", CASES)
def test_envelope_the_oracles_padded_tree_loses_no_aimed_ray(oracle, mesh_name, inst_name):
    """On every family and instance the GPU tests use: the oracle's walk of its own padded tree equals its brute-force form in found,
    item, face and the bits of toi.  Scenes of <= 50 items, so the oracle's item tree stays out of it.  No ray is excused; a G cell
    that fails here is D12 territory and leaves the generator as a whole (aimed_rays.DROPPED_G_CELLS)."""
    fs = ar.scene(mesh_name, inst_name)
    assert len(fs.items) <= 50
    cs = fs.c_struct()
    for family in ar.FAMILIES:
        R = ar.rays(mesh_name, inst_name, family)
        if not len(R):
            continue
        b = _brute(oracle, mesh_name, inst_name, family)
        t = oracle.trace_rays(cs, R.o, R.d, 1, brute_force=False)
        for label in np.unique(R.label):
            m = R.label == label
            bad = np.flatnonzero(m & ((b[0] != t[0]) | (b[0] & ((b[1] != t[1]) | (b[2] != t[2]) | (b[3].view(np.uint32) != t[3].view(np.uint32))))))
            assert len(bad) == 0, (mesh_name, inst_name, label, len(bad), int(m.sum()), bad[:5], R.o[bad[:2]], R.d[bad[:2]])
        assert not (b[0] & R.must_miss).any(), (mesh_name, inst_name, family)     # rays in the plane of a planar mesh miss


def test_every_family_reaches_every_mesh_it_is_defined_for():
    n = {(m, f): len(ar.rays(m, "identity", f)) for m in ar.MESHES for f in ar.FAMILIES}
    for m in ar.EXACT_MESHES:
        assert all(n[m, f] > 0 for f in ("V", "E", "U", "P", "A")), n
    assert n["soup", "E"] > 0 and n["soup", "U"] > 0 and n["soup", "A"] > 0 and n["soup", "G"] > 0 and n["lattice", "G"] > 0
    assert len(ar.DROPPED_G_CELLS) + len(np.unique(ar.rays("soup", "identity", "G").label)) == len(ar.G_SINES) * len(ar.G_DISTANCES)
    for m in ar.MESHES:
        for i in ar.INSTANCES:
            R = ar.all_rays(m, i)
            assert 500 < len(R) <= 50000, (m, i, len(R))
            assert np.isfinite(R.o).all() and np.isfinite(R.d).all()
            s, p = R.sorted_order(), R.permuted_order()
            assert sorted(set(s.tolist())) == sorted(p.tolist()) == list(range(len(R))) and len(s) < len(R) + 9 * 64
    a = ar.rays("cube", "identity", "A")
    zero = a.d == 0
    assert (zero & np.signbit(a.d)).any() and (zero & ~np.signbit(a.d)).any()      # either sign of zero
    assert (np.abs(a.o * 4 - np.round(a.o * 4)) == 0).all(axis=1).any()              # origins on lattice coordinates


@pytest.mark.parametrize("family", ["U", "G"])
def test_effectiveness_hits_and_misses(oracle, family):
    """At least a quarter of the rays of U and of G hit and at least a quarter miss: they sit ON the boundary between the two."""
    hit = total = 0
    for mesh_name in ar.MESHES:
        for inst_name in ar.INSTANCES:
            R = ar.rays(mesh_name, inst_name, family)
            if len(R):
                hit += int(_brute(oracle, mesh_name, inst_name, family)[0].sum()); total += len(R)
    assert total > 0 and 0.25 <= hit / total <= 0.75, (family, hit, total)
