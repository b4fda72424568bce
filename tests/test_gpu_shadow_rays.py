"""Ray-level parity of the SHADOW walk: every Raytracing::trace(ray, true, true, depth) call the oracle makes while rendering a
window is replayed through rr_trace_shadow_rays, with no limit and with limits built around the oracle's own toi, and the record
of every ray -- occluded, deciding item, face id, the bits of toi -- must be the reference's.  The walk is the one the frames'
shadow kernel uses (trace_shadow_packet / trace_shadow_ray): the skip of items beyond the light, the blocker pass, the NaN ball
and the packet form for 17 .. 512 items are pinned here below the pixel level, where a wrong occluder cannot hide behind a small
light term.  tests/shadow_ray_cases.py holds the cases and the expected value."""
import ctypes as C

import numpy as np
import pytest

from tests import shadow_ray_cases as cases
from tests.packet_pad import pad_inert

pytestmark = pytest.mark.gpu

FOUND_CLASSES = ("none", "t", "two_t", "1e30")     # occluded exactly where the oracle found something
SHORT_CLASSES = ("below_t", "half_t", "zero")      # occluded only where the oracle's toi is NaN


def _replay(ds, name, fs, rays, only=None):
    """Every limit class (or those of `only`) at every depth; returns class -> number of occluded rays."""
    cls = cases.limit_classes(fs, rays)
    n_occ = {}
    for cname, L in cls.items():
        if only is not None and cname not in only:
            continue
        n_occ[cname] = 0
        for depth, idx in cases.by_depth(rays):
            sub = cases.subset(rays, idx)
            lim = None if L is None else L[idx]
            got = ds.trace_shadow_rays(sub["origin"], sub["dir"], lim, depth)
            bad = cases.mismatches(got, sub, lim)
            assert len(bad) == 0, cases.describe(f"{name} / {cname} / depth {depth}", sub, lim, bad, got)
            n_occ[cname] += int(got[0].sum())
    return n_occ


def _both_outcomes_where_expected(n_occ, rays):
    n_found, n_nan = int(rays["found"].sum()), int((rays["found"] & np.isnan(rays["toi"])).sum())
    for c in FOUND_CLASSES:
        assert n_occ[c] == n_found, (c, n_occ[c], n_found)
    for c in SHORT_CLASSES:
        assert n_occ[c] == n_nan, (c, n_occ[c], n_nan)


@pytest.mark.parametrize("form", ["as_is", "packet_40_switches", "over_64_candidates"])
def test_shadow_rays_of_a_rendered_window(hip, oracle, form):
    """spheres_room: 14 items, the per-ray walk; padded to 40 items with the scene-wide switches (packet form, dividing inverse,
    alpha-occluder switch, NaN balls); padded to 100 copies (packets past 64 candidates fall back).  The decoys are invisible:
    the oracle's log of the padded scene is the unpadded one's."""
    fs, rays = cases.spheres_room_case(oracle)
    assert len(rays["toi"]) == 109248 and rays["found"].all() and sorted(set(rays["depth"].tolist())) == [1, 2, 3, 4, 5]
    scene = {"as_is": lambda: fs, "packet_40_switches": lambda: pad_inert(fs, 40, "switches"), "over_64_candidates": lambda: pad_inert(fs, 100, "copies")}[form]()
    with hip.DeviceScene(scene, 0) as ds:
        n_occ = _replay(ds, f"spheres_room {form}", fs, rays)
    _both_outcomes_where_expected(n_occ, rays)
    lights = [c for c in n_occ if c.startswith("light")]
    assert len(lights) == 3
    for c in lights:   # the distance a frame passes splits the rays: both outcomes occur
        assert 60000 <= n_occ[c] <= 72000, (c, n_occ[c])


@pytest.mark.parametrize("n_items", [1, 17])
def test_mesh_occluder_reports_the_nearest_hit(hip, oracle, n_items):
    """monkey: the deciding item is a mesh without an alpha map, which the walk only asks for ANY hit; the reported toi and face
    id come from the extra nearest-hit walk of that one item."""
    fs, rays = cases.monkey_case(oracle)
    assert len(rays["toi"]) == 1902 and int(rays["found"].sum()) == 1467 and rays["face"][rays["found"]].max() > 0
    scene = fs if n_items == len(fs.items) else pad_inert(fs, n_items, "copies")
    with hip.DeviceScene(scene, 0) as ds:
        n_occ = _replay(ds, f"monkey {n_items}", fs, rays)
        got = ds.trace_shadow_rays(rays["origin"][rays["depth"] == 1], rays["dir"][rays["depth"] == 1], None, 1)
    _both_outcomes_where_expected(n_occ, rays)
    assert got[0].any() and (~got[0]).any() and got[2][got[0]].max() > 0   # face ids above 0 were reported


CORNERS = ["blocker", "alpha_occluder", "projective", "deep_mesh", "inside_spheres_1.0_1", "inside_spheres_1.0_0", "inside_spheres_0.6_1"]


@pytest.mark.parametrize("name", CORNERS)
def test_corner_scenes(hip, oracle, name):
    fs, rays = cases.corner_case(oracle, name)
    assert rays["found"].any()
    with hip.DeviceScene(fs, 0) as ds:
        n_occ = _replay(ds, name, fs, rays)
    _both_outcomes_where_expected(n_occ, rays)


@pytest.mark.parametrize("n_items,mode", [(16, "copies"), (17, "copies"), (512, "copies"), (513, "copies"), (40, "switches")])
def test_blocker_pass_at_the_edges_of_the_packet_form(hip, oracle, n_items, mode):
    """blocker: a sphere BEHIND the point light precedes, in bbox-distance order, an occluder whose box reaches past the light.
    At the light's distance all 398 rays whose first item is that sphere are lit -- the rays the blocker pass exists for."""
    fs, rays = cases.corner_case(oracle, "blocker")
    assert len(fs.items) == 3 and int(rays["found"].sum()) == 398
    L = cases.limit_classes(fs, rays)["light0"]
    assert not cases.expected_occluded(rays, L).any() and (rays["found"] & (rays["toi"] > L)).sum() == 398
    scene = fs if n_items == len(fs.items) else pad_inert(fs, n_items, mode)
    with hip.DeviceScene(scene, 0) as ds:
        n_occ = _replay(ds, f"blocker {n_items} {mode}", fs, rays)
    _both_outcomes_where_expected(n_occ, rays)
    assert n_occ["light0"] == 0 and n_occ["none"] == 398


def test_nan_origin_stays_occluded_under_every_limit(hip, oracle):
    """tests/golden/fuzz_6601.npz: one shadow ray starts at a NaN point; the reference's first candidate ball answers Some(NaN),
    and `toi > len` is false for a NaN toi whatever the length."""
    fs, rays = cases.fuzz_6601_case(oracle)
    nan_ray = np.isnan(rays["origin"]).any(axis=1)
    assert nan_ray.sum() == 1 and rays["found"][nan_ray].all() and np.isnan(rays["toi"][nan_ray]).all()
    with hip.DeviceScene(fs, 0) as ds:
        n_occ = _replay(ds, "fuzz_6601", fs, rays)
        i = int(np.flatnonzero(nan_ray)[0])
        for cname, L in cases.limit_classes(fs, rays).items():
            occ, item, face, toi = ds.trace_shadow_rays(rays["origin"][i:i + 1], rays["dir"][i:i + 1], None if L is None else L[i:i + 1], int(rays["depth"][i]))
            assert occ[0] and item[0] == rays["item"][i] and face[0] == 0 and np.isnan(toi[0]), cname
    _both_outcomes_where_expected(n_occ, rays)
    assert n_occ["zero"] == 1


def test_order_of_the_rays_does_not_matter(hip, oracle):
    """The rays of the rendered window in log order (coherent packets: the packet form) and under one fixed permutation
    (incoherent packets: the per-ray walk): every ray gets the same record."""
    fs, rays = cases.spheres_room_case(oracle)
    perm = np.random.default_rng(0).permutation(len(rays["toi"]))
    shuffled = cases.subset(rays, perm)
    cls, cls_s = cases.limit_classes(fs, rays), cases.limit_classes(fs, shuffled)
    with hip.DeviceScene(pad_inert(fs, 40, "switches"), 0) as ds:
        for cname in ("none", "light1"):
            rec = {}
            for tag, r, c in (("log", rays, cls), ("shuffled", shuffled, cls_s)):
                out = np.zeros((len(r["toi"]), 4), np.uint32)
                for depth, idx in cases.by_depth(r):
                    lim = None if c[cname] is None else c[cname][idx]
                    occ, item, face, toi = ds.trace_shadow_rays(r["origin"][idx], r["dir"][idx], lim, depth)
                    out[idx] = np.stack([occ.astype(np.uint32), item.view(np.uint32), face, toi.view(np.uint32)], axis=1)
                rec[tag] = out
            unshuffled = np.zeros_like(rec["shuffled"])
            unshuffled[perm] = rec["shuffled"]
            assert np.array_equal(rec["log"], unshuffled), cname
            assert rec["log"][:, 0].any() and (cname == "none" or (rec["log"][:, 0] == 0).any())


def test_edits_are_seen(hip, oracle):
    """After rr_scene_update_item_flags hides the occluder of alpha_occluder, the call answers what the oracle answers for the
    edited flat scene."""
    from tests import corner_scenes
    fs, rays = cases.corner_case(oracle, "alpha_occluder")
    assert (rays["item"][rays["found"]] == 1).all() and rays["found"].sum() > 500
    edited = corner_scenes.builders()["alpha_occluder"]()
    edited.items[1].visible = False
    after = dict(rays)
    after["found"], after["item"], after["face"], after["toi"] = (a.copy() for a in (rays["found"], rays["item"], rays["face"], rays["toi"]))
    for depth, idx in cases.by_depth(rays):
        f, it, fc, t = oracle.trace_rays(edited.c_struct(), rays["origin"][idx], rays["dir"][idx], depth, for_shadow=True)
        after["found"][idx], after["item"][idx], after["face"][idx], after["toi"][idx] = f, it, fc, t
    assert int(after["found"].sum()) < int(rays["found"].sum())   # the edit changes the answers
    with hip.DeviceScene(fs, 0) as ds:
        before = _replay(ds, "alpha_occluder", fs, rays, only=("none",))
        ds.update_item_flags([it.visible for it in edited.items], [it.flip_normals for it in edited.items])
        n_occ = _replay(ds, "alpha_occluder, cover hidden", edited, after)
    assert before["none"] == int(rays["found"].sum())
    _both_outcomes_where_expected(n_occ, after)


def test_arguments(hip):
    from tests.helpers import load_scene
    fs = load_scene("spheres")
    o = np.zeros((4, 3), np.float32); d = np.tile(np.array([[0, 0, -1]], np.float32), (4, 1))
    with hip.DeviceScene(fs, 0) as ds:
        occ, item, face, toi = ds.trace_shadow_rays(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), None, 1)
        assert len(occ) == 0 and len(item) == 0
        # n == 0 touches nothing: not even NULL arrays
        assert hip.lib().rr_trace_shadow_rays(ds._h, None, None, None, 0, 1, None) == 0
        for depth in (0, 256):
            with pytest.raises(hip.RustrayHipError) as e:
                ds.trace_shadow_rays(o, d, None, depth)
            assert e.value.code == -1 and "depth" in str(e.value)
        for bad in (np.nan, -1.0, -np.inf):
            lim = np.array([1.0, 2.0, bad, bad], np.float32)
            with pytest.raises(hip.RustrayHipError) as e:
                ds.trace_shadow_rays(o, d, lim, 1)
            assert e.value.code == -1 and "max_distance[2]" in str(e.value), str(e.value)
        # +inf = the NULL form; -0.0 is a distance
        rng = np.random.default_rng(5)
        eye = np.asarray(fs.meta["camera"]["eye_pos"], np.float32)
        ro = (eye[None, :] + rng.normal(size=(512, 3)).astype(np.float32)).astype(np.float32)
        rd = rng.normal(size=(512, 3)).astype(np.float32)
        a = ds.trace_shadow_rays(ro, rd, None, 1)
        b = ds.trace_shadow_rays(ro, rd, np.full(512, np.inf, np.float32), 1)
        assert a[0].any() and (~a[0]).any()
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
        ds.trace_shadow_rays(ro[:4], rd[:4], np.array([-0.0, 0.0, 1.0, 2.0], np.float32), 1)
        # a ray that points away from everything
        occ, item, face, toi = ds.trace_shadow_rays(np.array([[0, 1e6, 0]], np.float32), np.array([[0, 1, 0]], np.float32), None, 1)
        assert not occ[0] and item[0] == -1 and face[0] == 0 and toi[0] == 0.0


def _free_bytes():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]


def test_host_failure_returns_an_error_and_leaks_nothing(hip, oracle):
    """A host-side exception (the test-only fault hook, as tests/test_gpu_guard.py) next to the host staging of the rays: a status
    code comes back, the handle answers correctly afterwards, device memory does not grow."""
    fs, rays = cases.corner_case(oracle, "blocker")
    L = hip.lib()
    L.rr_test_fault.argtypes = [C.c_char_p, C.c_int, C.c_int]
    with hip.DeviceScene(fs, 0) as ds:
        n0 = _replay(ds, "blocker", fs, rays, only=("none", "light0"))   # first use: runtime allocations settle
        free0 = _free_bytes()
        try:
            for kind, code in ((1, -5), (2, -4)):
                assert L.rr_test_fault(b"trace_shadow_rays.host", kind, 0) == 0
                with pytest.raises(hip.RustrayHipError) as e:
                    ds.trace_shadow_rays(rays["origin"], rays["dir"], None, 1)
                assert e.value.code == code and "rr_trace_shadow_rays" in str(e.value), str(e.value)
        finally:
            assert L.rr_test_fault(b"", 0, 0) == 0
        assert _replay(ds, "blocker after the failures", fs, rays, only=("none", "light0")) == n0
        assert abs(_free_bytes() - free0) < (8 << 20)
