"""The item set-up of a candidate (rr_primitives.h ItemRec): a packet's candidate is one item for all 64 lanes, and its record
-- inverse rows, local box, flags, the group that names the mesh's tree -- is fetched once per wave through the scalar cache
(item_rec_uniform) where the per-ray walks read it per lane.  Nothing a ray hits may change by a bit.

The lever is tests/packet_pad.py, as in tests/test_gpu_packet_groups.py: the base scene has 7 items and takes the per-ray walk;
padded into 17 .. 512 items the same picture is traced by packets.  Frames are 32 x 16 at 64 samples with monte_carlo, so a
level-1 packet is the 64 samples of one pixel and shadow rays take fixed slots.  What this file adds: the projective w row
through the uniform loader (mode `switches`), the record after every kind of edit (a record kept from the frame before would
show here), every kind of candidate in one packet range, and both loaders against the oracle's all-items form at ray level."""
import copy

import numpy as np
import pytest

from rustray_amd.flat import Item, Material, MeshData, make_config
from rustray_amd.scene import Scene, get_transformation, inverse_affine
from tests import shadow_ray_cases as cases
from tests.helpers import assert_frames_identical, camera_for, item_transforms, with_transforms
from tests.packet_pad import PACKET_LANES, in_packet_range, pad_inert
from tests.test_gpu_packet_groups import _bundles, _shadow_bundles
from tests.test_gpu_packet_walk import _assert_hits_equal, lights_scene, packet_groups

pytestmark = pytest.mark.gpu
COUNTS = ("primary_rays", "secondary_rays", "shaded_hits", "shadow_rays")
W, H = 32, 16


def _cfg():
    return make_config(samples=64, monte_carlo=True, seed=5, max_recursion=3)


def _frame(ds, fs):
    out = ds.render(camera_for(fs, W, H).c_struct(), _cfg())
    st = ds.stats()
    return out, [st[k] for k in COUNTS]


def _render(hip, fs):
    with hip.DeviceScene(fs, 0) as ds:
        return _frame(ds, fs)


def _clone(fs):
    """A deep copy (without the buffers that a c_struct() view of `fs` borrows)."""
    return pad_inert(fs, len(fs.items), "copies")


@pytest.fixture(scope="module")
def base():
    fs = lights_scene()
    assert not in_packet_range(len(fs.items))
    return fs


@pytest.fixture(scope="module")
def reference(hip, base):
    """The unpadded scene's frame, by the per-ray walk: computed once."""
    out, counts = _render(hip, base)
    assert counts[3] > 0 and (out["object_id"] != 0).any()
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out, counts


@pytest.mark.parametrize("mode", ("scattered", "switches"))
@pytest.mark.parametrize("n", (17, 65))
def test_padded_frame_equals_unpadded_frame(hip, base, reference, n, mode):
    """RGBA8, normal, depth, object id and the four ray counts, at the first packet size and the first grouped one.  `switches`
    holds a projective inverse (the scene takes the dividing form of inverse_ray: the w row of every candidate is fetched) and an
    alpha-mapped occluder."""
    ref, counts0 = reference
    p = pad_inert(base, n, mode, seed=n)
    assert in_packet_range(len(p.items))
    out, counts = _render(hip, p)
    assert_frames_identical(out, ref, f"{mode} {n}")
    assert counts == counts0, (mode, n, counts, counts0)


def _both(fs, i, **kw):
    it = fs.items[i]
    for idx in (it.material, it.material_cache):
        for k, v in kw.items():
            setattr(fs.materials[idx], k, v)


def test_frames_after_edits_equal_fresh_scenes(hip, base):
    """One handle in packet range; between frames: rr_scene_update_transforms, a real occluder hidden, cast_shadow of another
    cleared, an item deleted and added again.  After each edit the frame and the ray counts equal those of a scene created in that
    state -- a candidate's record is read again in every launch."""
    p = pad_inert(base, 40, "scattered", seed=40)
    assert in_packet_range(len(p.items)) and in_packet_range(len(p.items) - 1)
    t, ti = item_transforms(p, dx=0.37)
    moved = with_transforms(p, t, ti)
    hidden = _clone(moved)
    hidden.items[1].visible = False              # the ball whose shadow the first light casts on the floor
    unshadowed = _clone(hidden)
    assert unshadowed.materials[unshadowed.items[2].material_cache].cast_shadow
    _both(unshadowed, 2, cast_shadow=False)
    deleted = _clone(unshadowed)
    del deleted.items[3]
    states = [("created", p), ("update_transforms", moved), ("occluder hidden", hidden), ("cast_shadow cleared", unshadowed),
              ("item deleted", deleted), ("item added again", unshadowed)]
    fresh = {what: _render(hip, _clone(fs)) for what, fs in states[:-1]}
    fresh["item added again"] = fresh["cast_shadow cleared"]
    frames = [fresh[what][0] for what, _ in states[:-1]]
    for a, b in zip(frames, frames[1:]):         # every edit changes the picture: a stale record could not pass
        assert any(not np.array_equal(a[k], b[k]) for k in ("rgba", "depth", "object_id"))
    with hip.DeviceScene(p, 0) as ds:
        for what, fs in states:
            if what == "update_transforms":
                ds.update_transforms(t, ti)
            elif what == "occluder hidden":
                ds.update_item_flags([it.visible for it in fs.items], [it.flip_normals for it in fs.items])
            elif what == "cast_shadow cleared":
                ds.update_materials(fs.materials)
            elif what in ("item deleted", "item added again"):
                ds.set_items(fs.items, fs.materials)
            out, counts = _frame(ds, fs)
            assert_frames_identical(out, fresh[what][0], what)
            assert counts == fresh[what][1], (what, counts, fresh[what][1])


def _kinds_scene():
    """lights_scene (five balls, two one-leaf quads) with a mesh that has no triangles and a single triangle, both in view."""
    fs = lights_scene()
    m = Material(base_color=(0.2, 0.9, 0.3))

    def add(mesh, centre, lo, hi, idn, name):
        fs.meshes.append(mesh)
        fs.materials.append(copy.deepcopy(m)); fs.materials.append(Scene._cache_of(m))
        t = get_transformation(np.eye(4, dtype=np.float32), centre, (1.0, 1.0, 1.0), (0.0, 0.3, 0.0))
        fs.items.append(Item(kind=1, id=idn, material=len(fs.materials) - 2, material_cache=len(fs.materials) - 1, mesh=len(fs.meshes) - 1,
                             trans=t, trans_inv=inverse_affine(t), bbox_min=lo, bbox_max=hi, name=name))

    add(MeshData(positions=np.zeros((0, 3), np.float32), indices=np.zeros((0, 3), np.uint32)), (0.0, 1.0, -2.0), (-1.5, -1.0, -1.5), (1.5, 1.0, 1.5), 40, "empty")
    add(MeshData(positions=np.asarray([[-1, 0, 0], [1, 0, 0], [0, 1.5, 0]], np.float32), indices=np.asarray([[0, 1, 2]], np.uint32)),
        (-2.0, 0.2, -4.0), (-1.0, 0.0, 0.0), (1.0, 1.5, 0.0), 41, "one_triangle")
    return fs


def test_every_kind_of_candidate(hip):
    """A ball, a mesh without triangles (root4 = the empty tree) and meshes of one leaf (root4 = a leaf code) among the candidates
    of the same packets: the padded frame equals the unpadded one."""
    fs = _kinds_scene()
    assert not in_packet_range(len(fs.items))
    ref, counts0 = _render(hip, _clone(fs))
    assert 41 in np.unique(ref["object_id"]).tolist()
    for n, mode in ((24, "scattered"), (66, "switches")):
        out, counts = _render(hip, pad_inert(fs, n, mode, seed=n))
        assert_frames_identical(out, ref, f"{mode} {n}")
        assert counts == counts0, (mode, n, counts, counts0)


def _mixed(d):
    """Every second ray of each bundle mirrored in x: no bundle shares its signs, so every ray takes the per-ray walk."""
    d = d.copy()
    d[1::2, 0] = -d[1::2, 0]
    return d


def test_both_loaders_against_the_oracle_at_ray_level(hip, oracle, base):
    """rr_trace_rays and rr_trace_shadow_rays on bundles of 64 rays: with shared signs (packets: the uniform loader) and with mixed
    signs (the per-ray walk: the per-lane loader), against the oracle's all-items form field for field (found / occluded, item,
    face, toi bits)."""
    rng = np.random.default_rng(13)
    o, d = _bundles(base, rng)
    so, sd, sl = _shadow_bundles(base, rng)
    assert packet_groups(o, d).all() and packet_groups(so, sd).all()
    assert not packet_groups(o, _mixed(d)).any() and not packet_groups(so, _mixed(sd)).any()
    for n, mode in ((24, "switches"), (65, "scattered")):
        p = pad_inert(base, n, mode, seed=n)
        c = p.c_struct()
        with hip.DeviceScene(p, 0) as ds:
            for what, dd, sdd in (("shared signs", d, sd), ("mixed signs", _mixed(d), _mixed(sd))):
                g = ds.trace_rays(o, dd, 1)
                assert g[0].mean() > 0.2
                _assert_hits_equal(g, oracle.trace_rays(c, o, dd, 1, brute_force=True), f"closest {mode} {n} {what}")
                f, it, fc, t = oracle.trace_rays(c, so, sdd, 1, for_shadow=True, brute_force=True)
                ref = dict(found=f, item=it, face=fc, toi=t)
                for lim in (None, sl):
                    got = ds.trace_shadow_rays(so, sdd, lim, 1)
                    bad = cases.mismatches(got, ref, lim)
                    assert len(bad) == 0, f"shadow {mode} {n} {what} limit {lim is not None}: {len(bad)} records differ, first {int(bad[0])}"
                if what == "shared signs":
                    assert got[0].sum() >= PACKET_LANES // 2 and not got[0].all()
