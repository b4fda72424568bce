"""The packet form of the top level (17 .. 512 items: rr_trace.h beam_candidates, trace_closest_packet, trace_shadow_packet and
the level-1 fixed shadow slots) against the per-ray walk and the oracle, on the cases built to break it.

The lever is tests/packet_pad.py: invisible decoys move a scene into (or out of) the packet range and fill packets past 64
candidates without changing what any ray hits (tests/test_packet_pad.py shows that in the oracle).  So the device frame of a
padded scene must equal its frame of the unpadded scene bit for bit.  Below the frame level, rr_trace_rays runs the closest-hit
kernel on rays laid out in packets of 64 (the last one repeats its final ray), and found / item / face / toi must equal the
oracle's all-items form bit for bit."""
import glob
import os

import numpy as np
import pytest

from rustray_amd.flat import FlatScene, Item, Light, Material, MeshData, make_config
from rustray_amd.scene import Scene, get_transformation, inverse_affine
from tests.corner_scenes import _quad, builders, equal_toi_scene
from tests.helpers import GOLDEN, assert_frames_identical, camera_for, item_transforms, load_scene, with_transforms
from tests.packet_pad import MODES, PACKET_LANES, in_packet_range, pad_inert
from tests.test_gpu_parity import SMALL, assert_parity

pytestmark = pytest.mark.gpu
N_TOTALS = (16, 17, 64, 65, 512, 513)
RAYS = ("primary_rays", "secondary_rays", "shaded_hits")


# ---------------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------------
def _add(fs, item, m):
    fs.materials.append(m); fs.materials.append(Scene._cache_of(m))
    item.material, item.material_cache = len(fs.materials) - 2, len(fs.materials) - 1
    fs.items.append(item)


def _ball(fs, idn, centre, r, m, visible=True):
    t = get_transformation(np.eye(4, dtype=np.float32), tuple(float(v) for v in centre), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
    _add(fs, Item(kind=0, id=idn, material=0, material_cache=0, radius=r, trans=t, trans_inv=inverse_affine(t),
                  bbox_min=(-r,) * 3, bbox_max=(r,) * 3, visible=visible, name=f"ball{idn}"), m)


def _floor(fs, idn, y, half, m):
    fs.meshes.append(_quad(y, half))
    eye = np.eye(4, dtype=np.float32)
    _add(fs, Item(kind=1, id=idn, material=0, material_cache=0, mesh=len(fs.meshes) - 1, trans=eye.copy(), trans_inv=eye.copy(),
                  bbox_min=(-half, y, -half), bbox_max=(half, y, half), name=f"floor{idn}"), m)


def _camera(fs, eye, direction, fov=60.0):
    fs.meta = {"camera": dict(width=64, height=64, fov=float(np.float32(np.radians(fov))), eye_pos=list(eye), up=[0.0, 1.0, 0.0],
                              dir=list(direction), clipping_near=0.1, clipping_far=1000.0)}


def lights_scene():
    """Shadow packets under every light kind: a point light low over a floor (occluders nearer than the light and beyond it), a
    directional and a spot light (limit FLT_MAX), a disabled light between enabled ones, an alpha-mapped occluder."""
    fs = FlatScene()
    rng = np.random.default_rng(11)
    alpha = np.zeros((8, 8, 4), np.uint8); alpha[..., :3] = (rng.integers(0, 2, (8, 8, 1)) * 255).astype(np.uint8); alpha[..., 3] = 255
    fs.textures = [alpha]
    _floor(fs, 2, 0.0, 30.0, Material(base_color=(0.8, 0.8, 0.8)))
    for k, (x, z, r) in enumerate(((-1.0, -3.0, 0.4), (2.5, -6.0, 0.7), (-4.0, -12.0, 1.0), (6.0, -20.0, 1.5), (0.5, 1.5, 0.3))):
        _ball(fs, 10 + k, (x, r + 0.05 * k, z), r, Material(base_color=(0.3 + 0.1 * k, 0.5, 0.7), shininess=40.0))
    cover = _quad(0.0, 1.2)
    fs.meshes.append(cover)
    t = get_transformation(np.eye(4, dtype=np.float32), (1.5, 1.6, -4.0), (1.0, 1.0, 1.0), (0.3, 0.0, 0.2))
    am = Material(base_color=(0.9, 0.4, 0.2)); am.texture[4] = 0
    _add(fs, Item(kind=1, id=30, material=0, material_cache=0, mesh=len(fs.meshes) - 1, trans=t, trans_inv=inverse_affine(t),
                  bbox_min=(-1.2, 0.0, -1.2), bbox_max=(1.2, 0.0, 1.2), name="alpha_cover"), am)
    fs.lights = [Light(pos=(0.0, 1.2, -5.0), intensity=40.0),
                 Light(pos=(3.0, 4.0, 0.0), intensity=80.0, enabled=False),
                 Light(dir=(0.4, -1.0, -0.3), intensity=0.5, light_type=0, color=(1.0, 0.9, 0.8)),
                 Light(pos=(-3.0, 6.0, 2.0), dir=(0.3, -1.0, -0.8), intensity=150.0, light_type=2, max_angle=0.6),
                 Light(pos=(5.0, 0.8, -15.0), intensity=25.0, color=(0.5, 0.7, 1.0))]
    _camera(fs, (0.0, 3.0, 5.0), (0.0, -0.3, -1.0))
    return fs


def ball_field(n_side=(6, 5, 6), r=0.55):
    """Visible balls on a grid (180) over a floor: a packet whose rays spread over the field has more than 64 candidates that
    it can hit, items of high index among them."""
    fs = FlatScene()
    _floor(fs, 1, -1.0, 40.0, Material(base_color=(0.6, 0.6, 0.6)))
    idn = 2
    for i in range(n_side[0]):
        for j in range(n_side[1]):
            for k in range(n_side[2]):
                _ball(fs, idn, (2.0 * i - 5.0, 1.2 * j, -4.0 - 2.0 * k), r + 0.02 * ((i + j + k) % 5),
                      Material(base_color=(0.2 + 0.1 * i, 0.3 + 0.1 * j, 0.2 + 0.1 * k)))
                idn += 1
    fs.lights = [Light(pos=(0.0, 10.0, 0.0), intensity=200.0)]
    _camera(fs, (0.0, 2.5, 6.0), (0.0, -0.1, -1.0))
    return fs


def _turned(seed):
    from tests.test_gpu_item_boxes import _turned as turned
    return turned(seed)


def _random(seed):
    from tests.test_gpu_random import _random_scene
    return _random_scene(seed)


def _fixture(name):
    return lambda: load_scene(name)


def _golden(name):
    return lambda: FlatScene.load(os.path.join(GOLDEN, name + ".npz"))


def _frame_bases():
    """name -> (builder, w, h, config keywords, modes)"""
    out = {}
    for name, w, h, spp, mc, seed in SMALL:
        if f"fixture_{name}" not in out:
            f = min(1.0, 96.0 / max(w, h))
            out[f"fixture_{name}"] = (_fixture(name), int(w * f), int(h * f), dict(samples=min(spp, 4), monte_carlo=mc, seed=seed), MODES)
    for path in sorted(glob.glob(os.path.join(GOLDEN, "fuzz_*.npz"))):
        name = os.path.basename(path)[:-4]
        fs = FlatScene.load(path)
        if len(fs.items) <= 16:   # (fuzz_far_302574 is in the packet range as it is: test_d10_fixture_matches_the_item_tree_form)
            out[name] = (_golden(name), fs.meta["wh"][0], fs.meta["wh"][1], dict(fs.meta["kw"]), ("copies",))   # copies keep the extent (D10)
    for name, b in builders().items():
        kw = dict(samples=1, monte_carlo=False) if name == "blocker" else dict(samples=2, monte_carlo=True, seed=3)
        out[f"corner_{name}"] = (b, 96, 96, kw, MODES)
    for seed in (1000, 1003, 1007, 1011):
        out[f"random_{seed}"] = ((lambda s=seed: _random(s)), 64, 48, dict(samples=2, monte_carlo=True, seed=seed, max_recursion=4), MODES)
    out["lights"] = (lights_scene, 96, 64, dict(samples=2, monte_carlo=True, seed=5, max_recursion=3), MODES)
    return out


FRAME_BASES = _frame_bases()


def _render(hip, fs, cam, cfg):
    with hip.DeviceScene(fs, 0) as ds:
        out = ds.render(cam, cfg)
        st = ds.stats()
    return out, st


# ---------------------------------------------------------------------------------------------------------------------------
# 2 (and 4): packet vs per-ray walk at frame level
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", sorted(FRAME_BASES))
def test_padded_frame_equals_unpadded_frame(hip, oracle, base):
    """Every base scene has at most 16 items (the per-ray walk).  Padded to 16 (still per-ray), 17 and 64 (the packet form), 65
    (packets of copies past 64 candidates fall back per packet), 512 (the last packet range) and 513 (the per-ray walk again),
    in every decoy mode, the device frame stays the same bit for bit, and so do its ray and hit counts.  At 64 items the frame
    also matches the oracle's all-items form."""
    build, w, h, kw, modes = FRAME_BASES[base]
    fs = build()
    n0 = len(fs.items)
    assert n0 <= 16 and not in_packet_range(n0)
    cam = camera_for(fs, w, h).c_struct()
    cfg = make_config(**kw)
    ref, st0 = _render(hip, fs, cam, cfg)
    in_range = 0
    for n in N_TOTALS:
        for mode in modes:
            if n - n0 < (3 if mode == "switches" else 1):
                continue
            p = pad_inert(fs, n, mode, seed=n)
            out, st = _render(hip, p, cam, cfg)
            assert_frames_identical(out, ref, f"{base} {mode} {n}")
            assert [st[k] for k in RAYS] == [st0[k] for k in RAYS], (base, mode, n)
            in_range += in_packet_range(n)
            if n == 64 and mode == modes[0]:
                o = oracle.render(p.c_struct(), cam, cfg, want_means=True, n_threads=16, want_counters=True, brute_force=True)
                assert_parity(out, o, f"{base} {mode} {n}")
                c = o["counters"]
                assert [st[k] for k in RAYS] == [c["rays_primary"], c["rays_secondary"], c["shaded_hits"]], (base, mode, n)
    assert in_range >= 4 * len(modes)


def test_shadow_packets_under_every_light_kind(hip, oracle):
    """Part 2 traces shadow packets of the corner scenes (a point light over a floor with a blocker beyond it, an alpha-mapped
    occluder) and of lights_scene.  What it does not isolate: one light at a time.  Here each light kind of lights_scene is the
    only enabled light in its own frame (point low over the floor: limits from 0.3 to 30 units in one packet; directional and
    spot: limit FLT_MAX), and a disabled light sits between two enabled ones."""
    base = lights_scene()
    cam = camera_for(base, 48, 32).c_struct()
    cfg = make_config(samples=4, monte_carlo=True, seed=2, max_recursion=2)
    variants = {"point": [0], "directional": [2], "spot": [3], "disabled_between": [0, 4]}
    for what, on in variants.items():
        fs = pad_inert(base, len(base.items), "copies")
        for i, l in enumerate(fs.lights):
            l.enabled = i in on
        if what == "disabled_between":
            assert not fs.lights[1].enabled and fs.lights[0].enabled and fs.lights[4].enabled
        ref, st0 = _render(hip, fs, cam, cfg)
        for n in (24, 100):
            p = pad_inert(fs, n, "copies")
            assert in_packet_range(n)
            out, st = _render(hip, p, cam, cfg)
            assert_frames_identical(out, ref, f"{what} {n}")
            assert st["shadow_rays"] == st0["shadow_rays"] > 0 and [st[k] for k in RAYS] == [st0[k] for k in RAYS], what
        o = oracle.render(p.c_struct(), cam, cfg, want_means=True, n_threads=16, brute_force=True)
        assert_parity(out, o, what)


# ---------------------------------------------------------------------------------------------------------------------------
# 3: ray level
# ---------------------------------------------------------------------------------------------------------------------------
def packet_groups(o, d):
    """beam_candidates' coherence test, per group of 64 rays as k_trace_closest forms them (the lanes past the end repeat the
    last ray): finite origins and directions, |d_i| > 1e-30 and one sign per axis."""
    o, d = np.asarray(o, np.float32), np.asarray(d, np.float32)
    n = len(o)
    idx = np.minimum(np.arange(-(-n // PACKET_LANES) * PACKET_LANES), n - 1)
    O, D = o[idx].reshape(-1, PACKET_LANES, 3), d[idx].reshape(-1, PACKET_LANES, 3)
    finite = np.isfinite(O).all(axis=(1, 2)) & np.isfinite(D).all(axis=(1, 2))
    gate = (np.abs(D) > np.float32(1e-30)).all(axis=(1, 2))
    neg = D < 0
    one_sign = (neg.all(axis=1) | ~neg.any(axis=1)).all(axis=1)
    return finite & gate & one_sign


def _assert_hits_equal(g, r, what):
    assert np.array_equal(g[0], r[0]), (what, "found", np.nonzero(g[0] != r[0])[0][:10])
    f = g[0]
    bad = np.nonzero(g[1][f] != r[1][f])[0]
    assert len(bad) == 0, (what, "item", bad[:10], g[1][f][bad[:5]], r[1][f][bad[:5]])
    assert np.array_equal(g[2][f], r[2][f]), (what, "face")
    same = (g[3][f].view(np.uint32) == r[3][f].view(np.uint32)) | (np.isnan(g[3][f]) & np.isnan(r[3][f]))
    assert same.all(), (what, "toi", np.nonzero(~same)[0][:10])


def _trace(hip, oracle, fs, o, d, what, depth=1, ds=None):
    o, d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
    if ds is None:
        with hip.DeviceScene(fs, 0) as h:
            g = h.trace_rays(o, d, depth)
    else:
        g = ds.trace_rays(o, d, depth)
    r = oracle.trace_rays(fs.c_struct(), o, d, depth, brute_force=True)
    _assert_hits_equal(g, r, what)
    return g, r


def camera_block_rays(fs, w, h, block=8):
    """Pinhole rays through pixel centres, laid out in block x block tiles (one packet per 8x8 tile)."""
    cam = camera_for(fs, w, h)
    pi, vi = np.asarray(cam.projection_inverse, np.float64), np.asarray(cam.view_inverse, np.float64)
    o, d = [], []
    for by in range(0, h, block):
        for bx in range(0, w, block):
            ys, xs = np.mgrid[by:by + block, bx:bx + block]
            ndc = np.stack([(xs.ravel() + 0.5) / w * 2 - 1, 1 - (ys.ravel() + 0.5) / h * 2, -np.ones(xs.size), np.ones(xs.size)])
            p = pi @ ndc
            dc = p[:3] / p[3]
            dw = (vi[:3, :3] @ dc).T
            d.append(dw / np.linalg.norm(dw, axis=1, keepdims=True))
            o.append(np.broadcast_to(vi[:3, 3], dw.shape))
    return np.concatenate(o).astype(np.float32), np.concatenate(d).astype(np.float32)


def _world_vertices(fs, it):
    p = np.asarray(fs.meshes[it.mesh].positions, np.float64)
    t = np.asarray(it.trans, np.float64)
    return p @ t[:3, :3].T + t[:3, 3]


def grazing_rays(fs, eye, rng, spread=1e-3):
    """Per visible mesh item and axis: 64 rays from a narrow region around `eye` at the world vertex that reaches the item's min
    (max) along the axis, and at points 1 and 4 f32 ulps inward and outward of it along that axis.  Per zero-thickness item
    (a floor quad): 64 rays that skim it at grazing angles."""
    eye = np.asarray(eye, np.float64)
    steps = np.asarray([-4, -1, 0, 1, 4] * 13)[:PACKET_LANES]
    O, D = [], []
    for it in fs.items:
        if it.kind != 1 or not it.visible:
            continue
        v = _world_vertices(fs, it)
        ext = v.max(0) - v.min(0)
        for a in range(3):
            for side, k in ((-1.0, int(np.argmin(v[:, a]))), (1.0, int(np.argmax(v[:, a])))):
                tgt = np.repeat(v[k][None], PACKET_LANES, 0)
                ca = np.float32(tgt[0, a])
                tgt[:, a] = ca.astype(np.float64) + side * steps * np.spacing(np.abs(ca)).astype(np.float64)   # + outward, - inward
                o = eye + rng.uniform(-spread, spread, (PACKET_LANES, 3))
                O.append(o); D.append(tgt - o)
            if ext[a] <= 1e-6 * max(ext.max(), 1e-30):   # zero thickness along a: skim it
                lo, hi = v.min(0), v.max(0)
                up = np.zeros(3); up[a] = 1.0 if eye[a] >= lo[a] else -1.0
                far = lo + rng.uniform(0.6, 0.95, (PACKET_LANES, 3)) * (hi - lo)
                far[:, a] = lo[a]
                start = lo + rng.uniform(0.05, 0.1, 3) * (hi - lo)
                o = start + up * 1e-3 * ext.max() + rng.uniform(-spread, spread, (PACKET_LANES, 3)) * ext.max()
                o[:, a] = lo[a] + up[a] * 1e-3 * ext.max()
                O.append(o); D.append(far - o)
    return np.concatenate(O).astype(np.float32), np.concatenate(D).astype(np.float32)


def _ray_scenes():
    return {"spheres_room_copies_40": lambda: pad_inert(load_scene("spheres_room"), 40, "copies"),
            "kbert_room_scattered_100": lambda: pad_inert(load_scene("kbert_room"), 100, "scattered", seed=5),
            "random_1005_switches_200": lambda: pad_inert(_random(1005), 200, "switches"),
            "turned_sponza_41": lambda: _turned(41)}


RAY_SCENES = _ray_scenes()


@pytest.mark.parametrize("scene", sorted(RAY_SCENES))
def test_packets_at_ray_level(hip, oracle, scene):
    """a. 8x8 pixel blocks over the frustum; b. silhouette-grazing packets (the surface boxes' padding, k_item_spans' spans) and
    rays that skim zero-thickness items; e. batch lengths of 1 and 63 modulo 64 (the last packet repeats its final ray)."""
    fs = RAY_SCENES[scene]()
    assert in_packet_range(len(fs.items))
    rng = np.random.default_rng(len(fs.items))
    eye = np.asarray(fs.meta["camera"]["eye_pos"], np.float64)
    with hip.DeviceScene(fs, 0) as ds:
        o, d = camera_block_rays(fs, 64, 64)
        m = packet_groups(o, d)
        assert m.mean() >= 0.75, np.nonzero(~m)  # the 8x8 tiles are coherent packets, but those across a view axis where a direction changes sign
        _trace(hip, oracle, fs, o, d, f"{scene} camera tiles", ds=ds)
        o, d = o[np.repeat(m, PACKET_LANES)], d[np.repeat(m, PACKET_LANES)]
        go, gd = grazing_rays(fs, eye, rng)
        m = packet_groups(go, gd)
        assert m.mean() > 0.6, m.mean()          # most grazing groups take the packet form; those at an axis through the eye fall back
        _trace(hip, oracle, fs, go, gd, f"{scene} grazing", ds=ds)
        for n in (5 * PACKET_LANES + 1, 5 * PACKET_LANES + 63):
            assert packet_groups(o[:n], d[:n]).all() and n % PACKET_LANES in (1, 63)
            _trace(hip, oracle, fs, o[:n], d[:n], f"{scene} {n} rays", ds=ds)
            _trace(hip, oracle, fs, go[-n:], gd[-n:], f"{scene} {n} grazing rays", ds=ds)


def test_replayed_window_of_a_padded_scene(hip, oracle):
    """a. Every closest-hit ray the oracle traces for a window of a padded scene (40 items: the oracle's all-items form, <= 50),
    primary and secondary, replayed through rr_trace_rays (test_gpu_trace_rays.py: _replay)."""
    from tests.test_gpu_trace_rays import _replay
    fs = pad_inert(load_scene("spheres_room"), 40, "copies")
    assert in_packet_range(len(fs.items)) and len(fs.items) <= 50
    cam = camera_for(fs, 64, 48).c_struct()
    _, rays, n = _replay(hip, oracle, fs, cam, make_config(samples=4, monte_carlo=True, seed=8, max_recursion=4), (16, 8, 48, 40))
    assert n > 32 * 32 * 4 and rays["depth"].max() >= 3
    # the log's order makes few coherent packets: the same rays again, grouped by direction octant (then by direction)
    closest = ~rays["for_shadow"]
    with hip.DeviceScene(fs, 0) as ds:
        for depth in sorted(set(rays["depth"][closest].tolist())):
            m = np.nonzero(closest & (rays["depth"] == depth))[0]
            d = rays["dir"][m]
            m = m[np.lexsort((d[:, 1], d[:, 0], (d < 0) @ np.asarray([1, 2, 4])))]
            o, d = rays["origin"][m], rays["dir"][m]
            if depth == 1:
                assert packet_groups(o, d).mean() > 0.9
            g = ds.trace_rays(o, d, int(depth))
            _assert_hits_equal(g, (rays["found"][m], rays["item"][m], rays["face"][m], rays["toi"][m]), f"sorted depth {depth}")


def test_the_direction_gate(hip, oracle):
    """c. One packet per value of one direction component: +-1e-30 (the gate: |d| > 1e-30 takes the packet form), its neighbours
    on either side, +-0, +-subnormal; and packets where a single lane is off the gate (a 1e-30 component, a NaN, a flipped sign)."""
    fs = pad_inert(load_scene("spheres_room"), 40, "scattered", seed=3)
    assert in_packet_range(len(fs.items))
    rng = np.random.default_rng(3)
    eye = np.asarray(fs.meta["camera"]["eye_pos"], np.float32)
    tiny = np.float32(1e-30)
    values = [tiny, -tiny, np.nextafter(tiny, np.float32(0)), np.nextafter(tiny, np.float32(1)), -np.nextafter(tiny, np.float32(1)),
              np.float32(0.0), np.float32(-0.0), np.float32(1e-42), np.float32(-1e-42)]
    O, D, want = [], [], []
    for axis in range(3):
        for v in values:
            d = (np.asarray([0.3, -0.4, -1.0]) + rng.uniform(-0.05, 0.05, (PACKET_LANES, 3))).astype(np.float32)
            d[:, axis] = v
            O.append(eye + rng.uniform(-0.01, 0.01, (PACKET_LANES, 3)).astype(np.float32)); D.append(d)
            want.append(bool(abs(v) > tiny))
        base = np.asarray([0.3, 0.4, -1.0])
        for odd in (tiny, np.float32(np.nan), np.float32(-0.3 * np.sign(base[axis]))):
            d = (base + rng.uniform(-0.05, 0.05, (PACKET_LANES, 3))).astype(np.float32)
            d[int(rng.integers(0, PACKET_LANES)), axis] = odd
            O.append(eye + rng.uniform(-0.01, 0.01, (PACKET_LANES, 3)).astype(np.float32)); D.append(d)
            want.append(False)
    O, D = np.concatenate(O), np.concatenate(D)
    assert packet_groups(O, D).tolist() == want and sum(want) == 6
    _trace(hip, oracle, fs, O, D, "direction gate")


def _hit_box_count(fs, o, d):
    """Items whose world box (of the corners of the declared box) at least one of the rays passes, in float64: a lower bound on
    the candidates of the packet's interval ray."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    n = 0
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / d
        for it in fs.items:
            c = np.asarray([[(it.bbox_max if k & (1 << a) else it.bbox_min)[a] for a in range(3)] for k in range(8)], np.float64)
            w = c @ np.asarray(it.trans, np.float64)[:3, :3].T + np.asarray(it.trans, np.float64)[:3, 3]
            t0, t1 = (w.min(0) - o) * inv, (w.max(0) - o) * inv
            tn, tf = np.minimum(t0, t1).max(1), np.maximum(t0, t1).min(1)
            n += bool(((tn <= tf) & (tf >= 0)).any())
    return n


def test_candidate_count(hip, oracle):
    """d. 180 visible balls: packets whose origins spread across the field have more than 64 candidates (the wave falls back to the
    per-ray walk; a list cut at 64 would lose the balls of high index), packets from a narrow origin region fewer."""
    fs = ball_field()
    assert in_packet_range(len(fs.items)) and len(fs.items) > 2 * PACKET_LANES
    rng = np.random.default_rng(17)
    spread_o, spread_d, narrow_o, narrow_d = [], [], [], []
    for _ in range(24):
        o = np.stack([rng.uniform(-7, 3, PACKET_LANES), rng.uniform(0, 6, PACKET_LANES), np.full(PACKET_LANES, 6.0)], 1)
        d = np.stack([rng.uniform(0.01, 0.5, PACKET_LANES), rng.uniform(-0.4, -0.01, PACKET_LANES), -np.ones(PACKET_LANES)], 1)
        spread_o.append(o); spread_d.append(d)
        c = np.asarray([rng.uniform(-4, 4), rng.uniform(0.5, 4), 6.0])
        narrow_o.append(c + rng.uniform(-1e-3, 1e-3, (PACKET_LANES, 3)))
        narrow_d.append(np.asarray([rng.uniform(0.01, 0.2), rng.uniform(-0.2, -0.01), -1.0]) + rng.uniform(-0.005, 0.005, (PACKET_LANES, 3)))
    counts = [_hit_box_count(fs, o, d) for o, d in zip(spread_o, spread_d)]
    assert min(counts) > PACKET_LANES, counts                  # more than 64 candidates: these packets fall back
    assert max(_hit_box_count(fs, o, d) for o, d in zip(narrow_o, narrow_d)) <= 16
    so, sd = np.concatenate(spread_o).astype(np.float32), np.concatenate(spread_d).astype(np.float32)
    no, nd = np.concatenate(narrow_o).astype(np.float32), np.concatenate(narrow_d).astype(np.float32)
    assert packet_groups(so, sd).all() and packet_groups(no, nd).all()
    with hip.DeviceScene(fs, 0) as ds:
        g, _ = _trace(hip, oracle, fs, so, sd, "spread", ds=ds)
        assert (g[1][g[0]] >= PACKET_LANES).sum() > 100        # hits on balls past the first 64 candidates
        _trace(hip, oracle, fs, no, nd, "narrow", ds=ds)
    cam = camera_for(fs, 96, 64).c_struct()
    cfg = make_config(samples=2, monte_carlo=True, seed=4, max_recursion=3)
    out, _ = _render(hip, fs, cam, cfg)
    assert_parity(out, oracle.render(fs.c_struct(), cam, cfg, want_means=True, n_threads=16, brute_force=True), "ball field")


def _far(fs, off=1e4, scale=1e3):
    """The scene moved by `off` and scaled by `scale` (tools/fuzz_parity.py far_and_scaled, fixed), and the map of ray origins."""
    import copy
    out = copy.deepcopy(fs)
    M = np.eye(4); M[:3, :3] *= scale; M[:3, 3] = off
    for it in out.items:
        t = (M @ np.asarray(it.trans, np.float64)).astype(np.float32)
        it.trans, it.trans_inv = t, np.linalg.inv(t.astype(np.float64)).astype(np.float32)
    return out, (lambda o: (np.asarray(o, np.float64) * scale + off).astype(np.float32))


@pytest.mark.parametrize("scene", ["spheres_room_copies_40", "turned_sponza_41"])
def test_packets_far_from_the_origin(hip, oracle, scene):
    """f. The same scene and rays moved by 1e4 and scaled by 1e3."""
    fs = RAY_SCENES[scene]()
    assert in_packet_range(len(fs.items))
    eye = np.asarray(fs.meta["camera"]["eye_pos"], np.float64)
    o, d = camera_block_rays(fs, 48, 48)
    go, gd = grazing_rays(fs, eye, np.random.default_rng(2))
    m = packet_groups(o, d)
    assert m.mean() >= 0.75                      # (tiles across a view axis fall back)
    far, move = _far(fs)
    o, go = move(o), move(go)
    assert (packet_groups(o, d) == m).all() and packet_groups(go, gd).mean() > 0.6
    with hip.DeviceScene(far, 0) as ds:
        _trace(hip, oracle, far, o, d, f"{scene} far tiles", ds=ds)
        _trace(hip, oracle, far, go, gd, f"{scene} far grazing", ds=ds)


def _ties_scene(thick):
    """test_gpu_corners' two coplanar items (red: id 3, index 0; green: id 6, index 1) with 16 more visible balls behind the camera."""
    fs = equal_toi_scene(thick)
    for k in range(16):
        _ball(fs, 100 + k, (-8.0 + k, 4.0, 14.0), 0.4, Material(base_color=(0.5, 0.5, 0.9)))
    assert in_packet_range(len(fs.items))
    return fs


def test_equal_toi_ties_in_the_packet_range(hip, oracle):
    """g. With equal toi the smaller (bbox distance, index) wins: the lower index for equal boxes, the thicker box otherwise; at frame
    and at ray level.  And the case where a packet VISITS the items in the other order: green's declared box is cut to x >= 0, so
    for a packet whose lanes start low over red at x < 0 and high over both, the packet's lower bound puts red first (0.5 units)
    and green second (its x face), while each high lane enters green's box first: green must win those lanes' ties."""
    for thick, want in ((False, {0, 3}), (True, {0, 6})):
        fs = _ties_scene(thick)
        cam = camera_for(fs, 96, 96).c_struct()
        cfg = make_config(samples=2, monte_carlo=True, seed=3)
        out, _ = _render(hip, fs, cam, cfg)
        assert_parity(out, oracle.render(fs.c_struct(), cam, cfg, want_means=True, n_threads=16), f"thick={thick}")
        assert set(np.unique(out["object_id"])) - {100 + k for k in range(16)} == want
        rng = np.random.default_rng(1)
        o = np.stack([rng.uniform(-4, 4, 256), np.full(256, 6.0), rng.uniform(-4, 4, 256)], 1).astype(np.float32)
        d = np.stack([rng.uniform(1e-3, 2e-3, 256), -np.ones(256), rng.uniform(1e-3, 2e-3, 256)], 1).astype(np.float32)
        assert packet_groups(o, d).all()
        g, _ = _trace(hip, oracle, fs, o, d, f"ties thick={thick}")
        assert g[0].all() and (g[1] == (1 if thick else 0)).all()
    fs = _ties_scene(True)
    fs.items[1].bbox_min = (0.0, -1.0, -5.0)
    low = np.stack([np.full(32, -1.0), np.full(32, 0.5), np.linspace(-2, 2, 32)], 1)
    high = np.stack([np.full(32, -1.0), np.full(32, 20.0), np.linspace(-2, 2, 32)], 1)
    o = np.concatenate([low, high]).astype(np.float32)
    d = np.repeat(np.asarray([[0.2, -1.0, 1e-3]], np.float32), PACKET_LANES, 0)
    assert packet_groups(o, d).all()
    g, r = _trace(hip, oracle, fs, o, d, "visit order against tie order")
    assert (r[1][:32] == 0).all() and (r[1][32:] == 1).all() and r[0].all()


def test_near_coincident_surfaces(hip, oracle):
    """h. A flat quad at y = 0 and a sloped quad whose box starts in front of it (for rays going down) while its surface at the rays'
    footprint lies 1e-6 .. 1e-3 (relative) behind it: the sloped item is visited first, and a packet key that is not a true lower
    bound of the flat quad's toi stops the walk before it."""
    O, D = [], []
    fs = FlatScene()
    _floor(fs, 1, 0.0, 1.0, Material(base_color=(0.8, 0.8, 0.8)))
    H = 10.0
    for k, rel in enumerate((1e-6, 3e-6, 1e-5, 3e-5, 1e-4, 1e-3)):
        delta, a, x0 = rel * H, 0.05, 4.0 * k - 10.0
        # the sloped quad: y = -delta + a (x - x0) over x in [x0 - 1, x0 + 1]; the flat quad under the footprint is a copy at x0
        p = np.asarray([[x0 - 1, -delta - a, 1], [x0 + 1, -delta + a, 1], [x0 + 1, -delta + a, -1], [x0 - 1, -delta - a, -1]], np.float32)
        fs.meshes.append(MeshData(positions=p, indices=np.asarray([[0, 1, 2], [0, 2, 3]], np.uint32)))
        eye = np.eye(4, dtype=np.float32)
        _add(fs, Item(kind=1, id=10 + k, material=0, material_cache=0, mesh=len(fs.meshes) - 1, trans=eye.copy(), trans_inv=eye.copy(),
                      bbox_min=tuple(p.min(0)), bbox_max=tuple(p.max(0)), name=f"sloped{k}"), Material(base_color=(0.9, 0.2, 0.2)))
        t = get_transformation(eye, (x0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
        _add(fs, Item(kind=1, id=30 + k, material=0, material_cache=0, mesh=0, trans=t, trans_inv=inverse_affine(t),
                      bbox_min=(-1.0, 0.0, -1.0), bbox_max=(1.0, 0.0, 1.0), name=f"flat{k}"), Material(base_color=(0.2, 0.9, 0.2)))
        o = np.stack([x0 + np.linspace(-1e-3, 1e-3, PACKET_LANES) * delta, np.full(PACKET_LANES, H),
                      np.linspace(-0.3, 0.3, PACKET_LANES)], 1)
        O.append(o); D.append(np.repeat([[1e-7, -1.0, 1e-7]], PACKET_LANES, 0))
    fs.items[0].visible = False   # (the quad at the origin only lends its mesh)
    fs = pad_inert(fs, 20, "scattered", seed=1)
    assert in_packet_range(len(fs.items))
    o, d = np.concatenate(O).astype(np.float32), np.concatenate(D).astype(np.float32)
    assert packet_groups(o, d).all()
    g, r = _trace(hip, oracle, fs, o, d, "near-coincident")
    flat = np.asarray([fs.items[i].name.startswith("flat") for i in r[1]])
    assert r[0].all() and flat.all()        # the nearer (flat) surface, although the sloped box is entered first


def test_packets_after_a_transform_update(hip, oracle):
    """i. rr_scene_update_transforms derives the surface boxes again on the device: the same batches on the updated handle equal a
    fresh handle of the moved scene and the oracle."""
    base = pad_inert(load_scene("kbert_room"), 48, "copies")
    assert in_packet_range(len(base.items))
    t, ti = item_transforms(base, dx=0.37)
    moved = with_transforms(base, t, ti)
    eye = np.asarray(base.meta["camera"]["eye_pos"], np.float64)
    o, d = camera_block_rays(base, 48, 48)
    go, gd = grazing_rays(moved, eye, np.random.default_rng(6))
    with hip.DeviceScene(base, 0) as ds:
        ds.update_transforms(t, ti)
        a = [ds.trace_rays(o, d, 1), ds.trace_rays(go, gd, 1)]
    with hip.DeviceScene(moved, 0) as ds:
        b = [ds.trace_rays(o, d, 1), ds.trace_rays(go, gd, 1)]
    for x, y in zip(a, b):
        _assert_hits_equal(x, y, "updated vs fresh")
    _assert_hits_equal(a[0], oracle.trace_rays(moved.c_struct(), o, d, 1, brute_force=True), "updated vs oracle")
    _assert_hits_equal(a[1], oracle.trace_rays(moved.c_struct(), go, gd, 1, brute_force=True), "updated grazing vs oracle")


# ---------------------------------------------------------------------------------------------------------------------------
# 5: D10
# ---------------------------------------------------------------------------------------------------------------------------
D10_PIXELS = [(51, 68)]   # (y, x) where the oracle's item-tree form and its all-items form differ


def test_d10_fixture_matches_the_item_tree_form(hip, oracle):
    """tests/golden/fuzz_far_302574.npz (tools/fuzz_parity.py far, seed 302574; 62 items: the packet range).  The device keeps the
    items whose PADDED world box a ray passes; one of the all-items form's candidates has non-finite own-space arithmetic and is not
    among them.  The device frame equals the oracle's item-tree form bit for bit, ray counts included, and differs
    from the all-items form in the one recorded pixel only.  Padded with copies (the extent stays), it stays the same."""
    fs = FlatScene.load(os.path.join(GOLDEN, "fuzz_far_302574.npz"))
    assert len(fs.items) == 62 and in_packet_range(len(fs.items))
    w, h = fs.meta["wh"]
    cam = camera_for(fs, w, h).c_struct()
    cfg = make_config(**fs.meta["kw"])
    out, st = _render(hip, fs, cam, cfg)
    tree = oracle.render(fs.c_struct(), cam, cfg, want_means=True, n_threads=16, want_counters=True)
    allf = oracle.render(fs.c_struct(), cam, cfg, n_threads=16, want_counters=True, brute_force=True)
    assert np.array_equal(out["rgba"], tree["rgba"]) and np.array_equal(out["object_id"], tree["object_id"])
    assert_parity(out, tree, "item-tree form")
    c = tree["counters"]
    assert [st[k] for k in RAYS] == [c["rays_primary"], c["rays_secondary"], c["shaded_hits"]]
    diff = np.argwhere((tree["rgba"] != allf["rgba"]).any(-1)).tolist()
    assert [tuple(p) for p in diff] == D10_PIXELS
    assert (allf["rgba"][51, 68, :3] == 255).all() and not (out["rgba"][51, 68, :3] == 255).all()
    for n in (64, 65, 512, 513):
        p, pst = _render(hip, pad_inert(fs, n, "copies"), cam, cfg)
        assert_frames_identical(p, out, f"302574 copies {n}")
        assert [pst[k] for k in RAYS] == [st[k] for k in RAYS]
