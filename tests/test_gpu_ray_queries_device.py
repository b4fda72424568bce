"""The device-buffer, stream-ordered forms of the three ray queries (rr_trace_rays_device, rr_trace_shadow_rays_device,
rr_shade_rays_device) against their host forms: once the stream is synchronised, out_dev holds byte for byte what the host form
writes for the same inputs on the same handle state.  The host forms are the device forms behind a staging copy, so what the two
share (the streaming kernels around the walks) is judged from outside too: test_host_forms_against_the_oracle.

Two scenes: spheres_room as it is (14 items: every ray walks the top level) and padded to 40 items with the scene-wide switches
(tests/packet_pad.py: the packet form of the top level, the dividing inverse, the alpha-occluder switch, an overflowing ball), the
form the shadow-ray tests use.  The rays are the oracle's own `trace` calls of a small rendered window (its ray log), tiled to the
sizes below, with non-finite rays written over fixed positions.  Device buffers are torch tensors: torch and the library share one
HIP runtime (tests/conftest.py)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from rustray_amd import renderer
from rustray_amd.flat import RR_ITEM_SPHERE, RR_LIGHT_DIRECTIONAL, Item, make_config
from tests import shadow_ray_cases as cases
from tests.helpers import assert_frames_identical, camera_for, item_transforms, load_scene, with_transforms
from tests.packet_pad import pad_inert

pytestmark = pytest.mark.gpu

# the packet (64) and workgroup (256) edges of the streaming kernels, and 274 workgroups of ONE round each: their grid is capped at 8
# workgroups per CU, so only a size past multi_processor_count * 8 * 256 makes the grid-stride loop go round again (_second_round_size)
SIZES = (1, 63, 64, 65, 256, 257, 70001)
N_MAX = SIZES[-1]
SENTINEL = 0x5a5a5a5a
COUNTERS = ("primary_rays", "secondary_rays", "shadow_rays", "shaded_hits")
# non-finite rays, and at 7 a ray that starts outside the room and points away from everything, at fixed positions (every n >= 65 holds
# some; 70 001 all): (position, origin or None, direction or None)
SPECIAL = ((5, (np.nan, 0.0, 0.0), None), (7, (0.0, 1e4, 0.0), (0.0, 1.0, 0.0)), (60, (0.0, np.inf, 0.0), None), (64, None, (0.0, 0.0, 0.0)), (200, None, (np.nan, 1.0, 0.0)),
           (256, (-np.inf, 1.0, 2.0), (np.inf, 0.0, 1.0)), (69999, (np.nan, np.nan, np.nan), (np.nan, np.nan, np.nan)))


# ---- scenes and rays (each built once per process) ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scene(form):
    fs = load_scene("spheres_room")
    assert len(fs.items) == 14
    if form == "per_ray_14":
        return fs
    if form == "packet_40":
        return pad_inert(fs, 40, "switches")
    raise KeyError(form)


@functools.lru_cache(maxsize=None)
def _log(oracle):
    """Every trace call of an oracle render of a 32 x 16 window of spheres_room (2 samples, Monte Carlo, max_recursion 4)."""
    fs = load_scene("spheres_room")
    cam = camera_for(fs, 96, 64).c_struct()
    cfg = make_config(samples=2, monte_carlo=True, seed=3, max_recursion=4)
    with oracle.ray_log(1 << 17) as log:
        oracle.render(fs.c_struct(), cam, cfg, window=(32, 24, 64, 40), n_threads=1)
        rays = log.rays()
    assert 2000 < len(rays["depth"]) < (1 << 17)
    return rays


@functools.lru_cache(maxsize=None)
def _rays(oracle, shadow: bool, special: bool = True):
    """N_MAX rays (origins, directions): the logged closest-hit or shadow rays in call order, tiled, the SPECIAL ones written over."""
    log = _log(oracle)
    m = log["for_shadow"] if shadow else ~log["for_shadow"]
    assert m.sum() > 1000
    idx = np.resize(np.flatnonzero(m), N_MAX)
    o, d = log["origin"][idx].copy(), log["dir"][idx].copy()
    if special:
        for pos, so, sd in SPECIAL:
            if so is not None:
                o[pos] = so
            if sd is not None:
                d[pos] = sd
    o.setflags(write=False); d.setflags(write=False)
    return o, d


def _light_distances(fs, o):
    """|light.pos - origin| in float32 for the first point or spot light; +inf (no limit) where it is not finite."""
    l = next(l for l in fs.lights if l.light_type != RR_LIGHT_DIRECTIONAL)
    with np.errstate(invalid="ignore", over="ignore"):
        diff = (np.asarray(l.pos, np.float32)[None, :] - o).astype(np.float32)
        dist = np.sqrt((diff * diff).sum(axis=1, dtype=np.float32)).astype(np.float32)
    return np.where(np.isfinite(dist), dist, np.float32(np.inf)).astype(np.float32)


# ---- the two forms, as raw records -------------------------------------------------------------------------------------------------
def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_trace(hip, ds, o, d, depth):
    out = np.full((len(o), 5), SENTINEL, np.uint32)
    hip._check(hip.lib().rr_trace_rays(ds._h, _p(o), _p(d), len(o), depth, _p(out)))
    return out


def host_shadow(hip, ds, o, d, lim, depth):
    out = np.full((len(o), 5), SENTINEL, np.uint32)
    hip._check(hip.lib().rr_trace_shadow_rays(ds._h, _p(o), _p(d), None if lim is None else _p(lim), len(o), depth,
                                              out.ctypes.data_as(C.POINTER(hip.rr_shadow_hit))))
    return out


def host_shade(hip, ds, cfg, o, d, n_results, rpr, ids):
    out = np.full((n_results, 8), SENTINEL, np.uint32)
    hip._check(hip.lib().rr_shade_rays(ds._h, C.byref(cfg), _p(o), _p(d), n_results, rpr, None if ids is None else _p(ids), _p(out), None))
    return out


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sentinel(n, words):
    return torch.full((n, words), SENTINEL, dtype=torch.int32, device="cuda")


def _back(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32)


def dev_trace(ds, o, d, depth):
    to, td, out = _dev(o), _dev(d), _sentinel(len(o), 5)
    ds.trace_rays_device(to.data_ptr(), td.data_ptr(), len(o), depth, out.data_ptr())
    return _back(out)


def dev_shadow(ds, o, d, lim, depth):
    to, td, tl, out = _dev(o), _dev(d), _dev(lim), _sentinel(len(o), 5)
    ds.trace_shadow_rays_device(to.data_ptr(), td.data_ptr(), None if tl is None else tl.data_ptr(), len(o), depth, out.data_ptr())
    return _back(out)


def dev_shade(ds, cfg, o, d, n_results, rpr, ids):
    to, td, out = _dev(o), _dev(d), _sentinel(n_results, 8)
    ti = None if ids is None else _dev(ids.view(np.int32))
    ds.shade_rays_device(cfg, to.data_ptr(), td.data_ptr(), n_results, rpr, None if ti is None else ti.data_ptr(), out.data_ptr())
    return _back(out)


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype == np.uint32
    assert np.array_equal(a, b), f"{what}: {int((a != b).any(axis=1).sum())} of {len(a)} records differ, first at {int(np.flatnonzero((a != b).any(axis=1))[0])}"


# ---- 1: byte identity with the host form -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["per_ray_14", "packet_40"])
def test_closest_hits_equal_the_host_form(hip, oracle, form):
    o, d = _rays(oracle, shadow=False)
    n_hit = n_miss = n_nan = 0
    with hip.DeviceScene(_scene(form), 0) as ds:
        for depth in (1, 2):
            for n in SIZES:
                want = host_trace(hip, ds, o[:n], d[:n], depth)
                got = dev_trace(ds, o[:n], d[:n], depth)
                _same(got, want, f"{form} depth {depth} n {n}")
                assert not (got == SENTINEL).all(axis=1).any()
                n_hit += int((got[:, 0] == 1).sum()); n_miss += int((got[:, 0] == 0).sum())
                n_nan += int(np.isnan(got[:, 4].copy().view(np.float32)).sum())
    assert n_hit > 0 and n_miss > 0 and n_nan > 0   # hits, the not-hit record and NaN distances (non-finite rays against balls) all occurred


@pytest.mark.parametrize("form", ["per_ray_14", "packet_40"])
def test_shadow_hits_equal_the_host_form(hip, oracle, form):
    o, d = _rays(oracle, shadow=True)
    fs = _scene(form)
    limits = {"null": None, "inf": np.full(N_MAX, np.inf, np.float32), "light": _light_distances(fs, o)}
    assert np.isfinite(limits["light"]).sum() > N_MAX // 2
    seen = {k: [0, 0] for k in limits}
    with hip.DeviceScene(fs, 0) as ds:
        for depth in (1, 2):
            for n in SIZES:
                for name, lim in limits.items():
                    L = None if lim is None else np.ascontiguousarray(lim[:n])
                    want = host_shadow(hip, ds, o[:n], d[:n], L, depth)
                    got = dev_shadow(ds, o[:n], d[:n], L, depth)
                    _same(got, want, f"{form} depth {depth} n {n} limits {name}")
                    seen[name][0] += int((got[:, 0] == 1).sum()); seen[name][1] += int((got[:, 0] == 0).sum())
                    if name == "inf":   # +inf is the NULL form
                        _same(got, dev_shadow(ds, o[:n], d[:n], None, depth), f"{form} depth {depth} n {n}: +inf vs NULL")
    assert all(a > 0 for a, _ in seen.values()) and seen["light"][1] > seen["null"][1]   # the light's distance lights rays the NULL form occludes


def test_overflowing_ball_nan_toi(hip, oracle):
    """A VISIBLE ball whose arithmetic overflows (radius 1e12 under a 1e-12 scale, tests/test_gpu_item_boxes.py): rays through it
    come back hit with a NaN toi, the same bits in both forms, closest and shadow."""
    from rustray_amd.scene import get_transformation, inverse_affine
    fs = load_scene("spheres_room")
    t = get_transformation(np.eye(4, dtype=np.float32), (4.0, 3.0, -3.0), (float(np.float32(1e-12)),) * 3, (0.3, 0.4, 0.5))
    fs.items.append(Item(kind=RR_ITEM_SPHERE, id=9001, material=fs.items[0].material, material_cache=fs.items[0].material_cache, radius=1e12,
                         trans=t, trans_inv=inverse_affine(t), bbox_min=(-1e12,) * 3, bbox_max=(1e12,) * 3, name="overflowing_ball"))
    ball = len(fs.items) - 1
    rng = np.random.default_rng(11)
    n = 257
    o = (np.asarray([4.0, 3.0, -1.0], np.float32)[None, :] + rng.normal(scale=0.05, size=(n, 3))).astype(np.float32)   # two units in front of it
    tgt = (np.asarray([4.0, 3.0, -3.0], np.float32)[None, :] + rng.normal(scale=0.4, size=(n, 3))).astype(np.float32)
    d = (tgt - o).astype(np.float32)
    with hip.DeviceScene(fs, 0) as ds:
        for depth in (1, 2):
            want, got = host_trace(hip, ds, o, d, depth), dev_trace(ds, o, d, depth)
            _same(got, want, f"closest depth {depth}")
            ws, gs = host_shadow(hip, ds, o, d, None, depth), dev_shadow(ds, o, d, None, depth)
            _same(gs, ws, f"shadow depth {depth}")
        nan_hits = (got[:, 0] == 1) & np.isnan(got[:, 4].copy().view(np.float32))
    assert nan_hits.any() and (got[nan_hits, 1] == ball).all()


@pytest.mark.parametrize("form", ["per_ray_14", "packet_40"])
def test_straight_against_the_oracle(hip, oracle, form):
    """One case per query goes to the oracle itself, as the host-form tests do: 257 logged rays (no special ones), depth 2."""
    n, depth = 257, 2
    fs = _scene(form)
    plain_fs = load_scene("spheres_room")            # the decoys are invisible: the oracle's answers are the unpadded scene's
    plain = plain_fs.c_struct()                      # (borrows plain_fs's arrays: the scene object must outlive the struct)
    ids = np.asarray([it.id for it in fs.items], np.uint32)
    with hip.DeviceScene(fs, 0) as ds:
        o, d = (a[:n] for a in _rays(oracle, shadow=False, special=False))
        found, item, face, toi = oracle.trace_rays(plain, o, d, depth)
        got = dev_trace(ds, o, d, depth)
        assert np.array_equal(got[:, 0].astype(bool), found) and found.any()
        f = found
        assert np.array_equal(got[f, 1].view(np.int32), item[f]) and np.array_equal(got[f, 3], face[f])
        assert np.array_equal(got[f, 4], toi[f].view(np.uint32)) and (got[~f, 1] == 0xffffffff).all() and np.array_equal(got[f, 2], ids[got[f, 1]])
        o, d = (a[:n] for a in _rays(oracle, shadow=True, special=False))
        found, item, face, toi = oracle.trace_rays(plain, o, d, depth, for_shadow=True)
        ref = dict(found=found, item=item, face=face, toi=toi)
        for lim in (None, _light_distances(fs, o)):
            g = dev_shadow(ds, o, d, lim, depth)
            rec = (g[:, 0].astype(bool), g[:, 1].copy().view(np.int32), g[:, 3].copy(), g[:, 4].copy().view(np.float32))
            bad = cases.mismatches(rec, ref, lim)
            assert len(bad) == 0, f"{form}: {len(bad)} shadow records differ from the oracle's, first {int(bad[0])}"
            occ = g[:, 0] == 1
            assert occ.any() and np.array_equal(g[occ, 2], ids[g[occ, 1]])   # the occluders' object ids came with them


# ---- 1b: the host forms against the oracle -----------------------------------------------------------------------------------------
def _second_round_size():
    """Rays that make the grid-stride loop of k_pack_rays / k_unpack_hits take a second round (524 545 on an MI355X)."""
    return torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256 + 257


@functools.lru_cache(maxsize=None)
def _logged(oracle, shadow: bool):
    """((depth, calls), (depth, calls)): the logged closest-hit or shadow calls of depth 1 and of the depth past 1 that has most of
    them (past 1 the candidate filter admits the reflection-only items), in call order, with the oracle's own answers (a query
    takes one depth for all its rays).  All finite."""
    log = _log(oracle)
    m = log["for_shadow"] if shadow else ~log["for_shadow"]
    per_depth = np.bincount(log["depth"][m].astype(np.int64))
    out = []
    for depth in (1, 2 + int(per_depth[2:].argmax())):
        idx = np.flatnonzero(m & (log["depth"] == depth))
        calls = {k: log[k][idx] for k in ("origin", "dir", "found", "item", "face", "toi")}
        assert len(idx) > 100 and np.isfinite(calls["origin"]).all() and np.isfinite(calls["dir"]).all()
        assert calls["found"].any()
        out.append((depth, calls))
    return tuple(out)


def _tiled(calls, n):
    """The logged calls tiled to n rays: the oracle's answers tile with them."""
    idx = np.resize(np.arange(len(calls["toi"])), n)
    return {k: np.ascontiguousarray(v[idx]) for k, v in calls.items()}


def _closest_equals_the_oracle(got, ref, ids, what):
    f = ref["found"]
    assert got.shape == (len(f), 5), what
    assert np.array_equal(got[:, 0], f.astype(np.uint32)), (what, "found")
    assert np.array_equal(got[f, 1].view(np.int32), ref["item"][f]) and np.array_equal(got[f, 3], ref["face"][f]), (what, "item / face")
    assert np.array_equal(got[f, 4], ref["toi"][f].view(np.uint32)) and np.array_equal(got[f, 2], ids[got[f, 1]]), (what, "toi / object id")
    assert np.array_equal(got[~f], np.broadcast_to(np.asarray([0, 0xffffffff, 0, 0, 0], np.uint32), got[~f].shape)), (what, "the not-hit record")


def _shadow_equals_the_oracle(got, ref, lim, ids, what):
    assert got.shape == (len(ref["found"]), 5), what
    rec = (got[:, 0].astype(bool), got[:, 1].copy().view(np.int32), got[:, 3].copy(), got[:, 4].copy().view(np.float32))
    bad = cases.mismatches(rec, ref, lim)
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(got)} shadow records differ from the oracle's, first {int(bad[0])}"
    occ = got[:, 0] == 1
    assert (got[:, 0] <= 1).all() and np.array_equal(got[occ, 2], ids[got[occ, 1]]) and (got[~occ, 2] == 0).all(), (what, "object ids")


@pytest.mark.parametrize("form", ["per_ray_14", "packet_40"])
def test_host_forms_against_the_oracle(hip, oracle, form):
    """The HOST closest-hit and shadow forms against the oracle's own logged answers, bit for bit, every ray compared: the host
    forms run through the device forms' streaming kernels, so the identity tests above no longer judge those from outside.  Sizes:
    the packet and workgroup edges, each at depth 1 and at a deeper one, and at depth 1 one that takes the kernels' grid-stride loop
    into its second round; there the two device forms are held to the same answers."""
    fs = _scene(form)                                   # (the decoys of packet_40 are invisible: the oracle's answers are the unpadded scene's)
    ids = np.asarray([it.id for it in fs.items], np.uint32)
    big = _second_round_size()
    with hip.DeviceScene(fs, 0) as ds:
        for (c_depth, closest), (s_depth, shadow) in zip(_logged(oracle, False), _logged(oracle, True)):
            for n in (1, 63, 64, 65, 256, 257) + ((big,) if c_depth == 1 else ()):
                ref = _tiled(closest, n)
                what = f"{form} closest depth {c_depth} n {n}"
                _closest_equals_the_oracle(host_trace(hip, ds, ref["origin"], ref["dir"], c_depth), ref, ids, "host " + what)
                if n == big:
                    _closest_equals_the_oracle(dev_trace(ds, ref["origin"], ref["dir"], c_depth), ref, ids, "device " + what)
                ref = _tiled(shadow, n)
                what = f"{form} shadow depth {s_depth} n {n}"
                for lim in (None, _light_distances(fs, ref["origin"])):
                    _shadow_equals_the_oracle(host_shadow(hip, ds, ref["origin"], ref["dir"], lim, s_depth), ref, lim, ids, "host " + what)
                    if n == big:
                        _shadow_equals_the_oracle(dev_shadow(ds, ref["origin"], ref["dir"], lim, s_depth), ref, lim, ids, "device " + what)


# ---- 2: radiance -------------------------------------------------------------------------------------------------------------------
def _shade_cfg():
    return make_config(samples=1, monte_carlo=True, seed=3, max_recursion=3)


@pytest.mark.parametrize("form", ["per_ray_14", "packet_40"])
def test_radiance_equals_the_host_form(hip, oracle, form):
    o, d = _rays(oracle, shadow=False)
    cfg = _shade_cfg()
    with hip.DeviceScene(_scene(form), 0) as ds:
        for n_results in (1, 65, 4099):
            for rpr in (1, 3):
                n = n_results * rpr
                ids_given = (np.arange(n_results, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(7)).astype(np.uint32)   # all 32 bits in use
                for ids in (None, ids_given):
                    want = host_shade(hip, ds, cfg, o[:n], d[:n], n_results, rpr, ids); wst = ds.stats()
                    got = dev_shade(ds, cfg, o[:n], d[:n], n_results, rpr, ids); gst = ds.stats()
                    _same(got, want, f"{form} {n_results} x {rpr} ids {'given' if ids is not None else 'NULL'}")
                    for k in COUNTERS + ("batches",):
                        assert gst[k] == wst[k], (k, gst, wst)
                    assert gst["primary_rays"] == n
        assert (got[:, 0:3] != 0).any() and (got[:, 7] != 0).any()   # something was shaded


def test_radiance_in_several_batches(hip, oracle):
    """A ray-memory budget that cuts 12 297 rays into three batches (as tests/test_gpu_shade_rays.py forces them): the batches read
    the caller's buffers where they are, at offsets that cut results apart."""
    o, d = _rays(oracle, shadow=False)
    cfg = _shade_cfg()
    n_results, rpr = 4099, 3
    n = n_results * rpr
    slack = 2 * 256 * (cfg.max_recursion + 1)           # plan_ray_batches: 2 * RR_BLOCK * (max_recursion + 1)
    with hip.DeviceScene(_scene("packet_40"), 0) as ds:
        whole = dev_shade(ds, cfg, o[:n], d[:n], n_results, rpr, None); st1 = ds.stats()
        ds.set_tuning(queue_budget_bytes=56 * (3 * 5000 + slack), shade_chunk_rays=65536)
        want = host_shade(hip, ds, cfg, o[:n], d[:n], n_results, rpr, None); wst = ds.stats()
        got = dev_shade(ds, cfg, o[:n], d[:n], n_results, rpr, None); gst = ds.stats()
    assert st1["batches"] == 1 and gst["batches"] == wst["batches"] >= 2
    _same(got, want, "batched: device form vs host form")
    _same(got, whole, "batched vs one batch")
    for k in COUNTERS:
        assert gst[k] == wst[k] == st1[k], (k, gst, wst, st1)


# ---- 3: reach ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("query", ["closest", "shadow", "shade"])
def test_far_origins_pad_the_top_level_as_the_host_form_does(hip, oracle, query):
    """Origins 1e6 out on one axis (both signs), one infinite and one NaN origin: the device form finds the reach on the device, the
    host form on the host; two fresh handles must answer alike and render the same frame afterwards (the top level was rebuilt
    the same way, and came back for the frame's camera)."""
    o, d = (a[:257].copy() for a in _rays(oracle, shadow=(query == "shadow"), special=False))
    o[3, 0] = 1e6; o[100, 0] = -1e6; o[17] = (np.inf, 0.0, 0.0); o[130, 1] = np.nan
    d[3] = (-1.0, 0.0, 0.0); d[100] = (1.0, 0.0, 0.0)     # the far rays look back at the scene
    fs = _scene("packet_40")
    cam = camera_for(fs, 32, 32).c_struct()
    cfg = make_config(samples=2, monte_carlo=True, seed=5, max_recursion=3)
    scfg = _shade_cfg()
    frames, recs = {}, {}
    for which in ("device", "host"):
        with hip.DeviceScene(fs, 0) as ds:
            if query == "closest":
                recs[which] = dev_trace(ds, o, d, 1) if which == "device" else host_trace(hip, ds, o, d, 1)
            elif query == "shadow":
                recs[which] = dev_shadow(ds, o, d, None, 1) if which == "device" else host_shadow(hip, ds, o, d, None, 1)
            else:
                recs[which] = dev_shade(ds, scfg, o, d, 257, 1, None) if which == "device" else host_shade(hip, ds, scfg, o, d, 257, 1, None)
            frames[which] = ds.render(cam, cfg)
    _same(recs["device"], recs["host"], query)
    assert_frames_identical(frames["device"], frames["host"], "the frame after the far query")
    with hip.DeviceScene(fs, 0) as ds:
        assert_frames_identical(frames["device"], ds.render(cam, cfg), "against a handle that never saw the far rays")


# ---- 4: bad limits -----------------------------------------------------------------------------------------------------------------
def test_bad_limits_are_refused_before_anything_is_written(hip, oracle):
    o, d = (a[:257] for a in _rays(oracle, shadow=True))
    lim = np.full(257, 2.0, np.float32)
    lim[70] = np.nan; lim[5] = -1.0
    with hip.DeviceScene(_scene("packet_40"), 0) as ds:
        to, td, tl, out = _dev(o), _dev(d), _dev(lim), _sentinel(257, 5)
        with pytest.raises(hip.RustrayHipError) as e:
            ds.trace_shadow_rays_device(to.data_ptr(), td.data_ptr(), tl.data_ptr(), 257, 1, out.data_ptr())
        assert e.value.code == -1 and "max_distance[5]" in str(e.value), str(e.value)
        assert (_back(out) == SENTINEL).all()
        lim2 = lim.copy(); lim2[5] = 1.0                  # NaN alone, further back
        tl2 = _dev(lim2)
        with pytest.raises(hip.RustrayHipError) as e:
            ds.trace_shadow_rays_device(to.data_ptr(), td.data_ptr(), tl2.data_ptr(), 257, 1, out.data_ptr())
        assert e.value.code == -1 and "max_distance[70]" in str(e.value), str(e.value)
        assert (_back(out) == SENTINEL).all()
        good = np.full(257, 2.0, np.float32)
        _same(dev_shadow(ds, o, d, good, 1), host_shadow(hip, ds, o, d, good, 1), "the query after the refused ones")


# ---- 5: stream order with torch ----------------------------------------------------------------------------------------------------
def test_stream_order_with_torch(hip, oracle):
    o, d = (a[:70001] for a in _rays(oracle, shadow=False))
    with hip.DeviceScene(_scene("packet_40"), 0) as ds:
        base_o, base_d = _dev(o), _dev(d)
        shift = torch.tensor([0.25, -0.125, 0.5], dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        with torch.cuda.stream(s1):
            # the rays are PRODUCED on this stream and not synchronised: the query must read them in stream order
            ro = (base_o * 0.5 + shift).contiguous()
            rd = (base_d * 2.0).contiguous()
            res = renderer.trace_rays_torch(ds, ro, rd, depth=1)
            n_hit = res["hit"].sum()                              # ... and its result is consumed in stream order
            item_sum = torch.where(res["hit"] == 1, res["item_index"], torch.zeros_like(res["item_index"])).sum()
        s1.synchronize()                                          # the one synchronisation
        assert res["records"].shape == (70001, 5) and res["records"].dtype == torch.int32 and res["distance"].dtype == torch.float32
        assert res["records"].is_cuda and res["item_index"].data_ptr() == res["records"].data_ptr() + 4   # views, no copy
        want = host_trace(hip, ds, ro.cpu().numpy(), rd.cpu().numpy(), 1)
        got = res["records"].cpu().numpy().view(np.uint32)
        _same(got, want, "rays produced on the stream")
        assert int(n_hit) == int((want[:, 0] == 1).sum()) > 0
        assert int(item_sum) == int(want[want[:, 0] == 1, 1].astype(np.int64).sum())
        # two calls back to back on two streams, no synchronisation in between: the handle's buffers are shared, the library serialises
        ro2, rd2 = base_o.clone(), base_d.clone()
        lim = torch.full((70001,), float("inf"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            a = renderer.trace_rays_torch(ds, ro2, rd2, depth=2)
        with torch.cuda.stream(s2):
            b = renderer.trace_shadow_rays_torch(ds, ro2, rd2, lim, depth=2)
            c = renderer.trace_rays_torch(ds, ro, rd, depth=2)
        torch.cuda.synchronize()
        _same(a["records"].cpu().numpy().view(np.uint32), host_trace(hip, ds, o, d, 2), "first stream")
        _same(b["records"].cpu().numpy().view(np.uint32), host_shadow(hip, ds, o, d, None, 2), "second stream, shadow")
        _same(c["records"].cpu().numpy().view(np.uint32), host_trace(hip, ds, ro.cpu().numpy(), rd.cpu().numpy(), 2), "second stream, closest")
        assert b["occluded"].dtype == torch.int32 and int(b["occluded"].sum()) > 0


def test_torch_wrappers_return_views_and_refuse_other_tensors(hip, oracle):
    o, d = (a[:195] for a in _rays(oracle, shadow=False))
    cfg = _shade_cfg()
    with hip.DeviceScene(_scene("per_ray_14"), 0) as ds:
        to, td = _dev(o), _dev(d)
        ids = torch.arange(65, dtype=torch.int32, device="cuda") * 3
        r = renderer.shade_rays_torch(ds, to, td, cfg, rays_per_result=3, stream_ids=ids)
        torch.cuda.synchronize()
        assert r["records"].shape == (65, 8) and r["records"].dtype == torch.float32 and r["color"].shape == (65, 3) and r["normal"].shape == (65, 3)
        assert r["object_id"].dtype == torch.int32 and r["depth"].data_ptr() == r["records"].data_ptr() + 12
        want = host_shade(hip, ds, cfg, o, d, 65, 3, (np.arange(65, dtype=np.uint32) * 3).astype(np.uint32))
        _same(r["records"].cpu().numpy().view(np.uint32), want, "shade_rays_torch")
        s = renderer.trace_shadow_rays_torch(ds, to, td, None, depth=1)
        torch.cuda.synchronize()
        _same(s["records"].cpu().numpy().view(np.uint32), host_shadow(hip, ds, o, d, None, 1), "trace_shadow_rays_torch")
        empty = renderer.trace_rays_torch(ds, to[:0], td[:0])
        assert empty["records"].shape == (0, 5)
        for bad_o, exc in ((to.cpu(), ValueError), (to.double(), TypeError), (to.t().contiguous().t(), ValueError), (to.reshape(-1), ValueError),
                           (o, TypeError)):
            with pytest.raises(exc):
                renderer.trace_rays_torch(ds, bad_o, td)
        with pytest.raises(ValueError):
            renderer.trace_rays_torch(ds, to, td[:100])
        with pytest.raises(ValueError):
            renderer.shade_rays_torch(ds, to[:194], td[:194], cfg, rays_per_result=3)
        with pytest.raises(TypeError):
            renderer.trace_shadow_rays_torch(ds, to, td, torch.zeros(195, dtype=torch.float64, device="cuda"))


# ---- 6: edit after enqueue ---------------------------------------------------------------------------------------------------------
def test_an_edit_waits_for_the_query_in_flight(hip, oracle):
    o, d = _rays(oracle, shadow=False)
    fs = _scene("per_ray_14")
    t, ti = item_transforms(fs, dx=0.4)
    with hip.DeviceScene(fs, 0) as ref:
        unedited = host_trace(hip, ref, o, d, 1)
    with hip.DeviceScene(with_transforms(load_scene("spheres_room"), t, ti), 0) as ref:
        edited = host_trace(hip, ref, o, d, 1)
    assert (unedited != edited).any()
    with hip.DeviceScene(fs, 0) as ds:
        dev_trace(ds, o[:64], d[:64], 1)                      # first use: the handle's buffers exist
        to, td, out = _dev(o), _dev(d), _sentinel(N_MAX, 5)
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        ds.trace_rays_device(to.data_ptr(), td.data_ptr(), N_MAX, 1, out.data_ptr(), st.cuda_stream)
        ds.update_transforms(t, ti)                           # at once: the edit must wait for what the query still reads
        _same(_back(out), unedited, "the query enqueued before the edit")
        _same(dev_trace(ds, o, d, 1), edited, "the same query after the edit")


# ---- 7: argument checks that never reach the device -----------------------------------------------------------------------------------
def test_argument_checks(hip, oracle):
    o, d = (a[:4] for a in _rays(oracle, shadow=False))
    L = hip.lib()
    cfg = _shade_cfg()
    with hip.DeviceScene(_scene("per_ray_14"), 0) as ds:
        to, td, out5, out8 = _dev(o), _dev(d), _sentinel(4, 5), _sentinel(4, 8)
        po, pd, p5, p8 = (C.c_void_p(x.data_ptr()) for x in (to, td, out5, out8))
        h = ds._h
        # NULL buffers with n > 0
        for args in ((None, pd, p5), (po, None, p5), (po, pd, None)):
            assert L.rr_trace_rays_device(h, args[0], args[1], 4, 1, args[2], None) == -1 and b"NULL" in L.rr_last_error()
            assert L.rr_trace_shadow_rays_device(h, args[0], args[1], None, 4, 1, args[2], None) == -1 and b"NULL" in L.rr_last_error()
        for args in ((None, pd, p8), (po, None, p8), (po, pd, None)):
            assert L.rr_shade_rays_device(h, C.byref(cfg), args[0], args[1], 4, 1, None, args[2], None, None) == -1 and b"NULL" in L.rr_last_error()
        assert L.rr_trace_rays_device(None, po, pd, 4, 1, p5, None) == -1
        assert L.rr_shade_rays_device(h, None, po, pd, 4, 1, None, p8, None, None) == -1
        # depth 0 and 256, rays_per_result 0 and beyond the table, max_recursion, the size bound: the host forms' codes
        for depth in (0, 256):
            assert L.rr_trace_rays_device(h, po, pd, 4, depth, p5, None) == L.rr_trace_rays(h, po, pd, 4, depth, p5) == -1 and b"depth" in L.rr_last_error()
            assert L.rr_trace_shadow_rays_device(h, po, pd, None, 4, depth, p5, None) == -1 and b"depth" in L.rr_last_error()
        assert L.rr_shade_rays_device(h, C.byref(cfg), po, pd, 4, 0, None, p8, None, None) == -1 and b"rays_per_result" in L.rr_last_error()
        assert L.rr_shade_rays_device(h, C.byref(cfg), po, pd, 1, 32767, None, p8, None, None) == -2 and b"rays_per_result" in L.rr_last_error()
        deep = make_config(samples=1, max_recursion=31)
        assert L.rr_shade_rays_device(h, C.byref(deep), po, pd, 4, 1, None, p8, None, None) == -2 and b"max_recursion" in L.rr_last_error()
        assert L.rr_trace_rays_device(h, po, pd, 0x7fffff01, 1, p5, None) == -2
        assert L.rr_trace_shadow_rays_device(h, po, pd, None, 0x7fffff01, 1, p5, None) == -2
        assert L.rr_shade_rays_device(h, C.byref(cfg), po, pd, 0x7fffff01, 1, None, p8, None, None) == -2
        # n == 0 returns RR_OK, looks at no pointer and writes nothing
        assert L.rr_trace_rays_device(h, None, None, 0, 1, None, None) == 0
        assert L.rr_trace_shadow_rays_device(h, None, None, None, 0, 1, None, None) == 0
        assert L.rr_shade_rays_device(h, C.byref(cfg), None, None, 0, 3, None, None, None, None) == 0
        assert L.rr_trace_rays_device(h, po, pd, 0, 1, p5, None) == 0 and L.rr_shade_rays_device(h, C.byref(cfg), po, pd, 0, 1, None, p8, None, None) == 0
        # a cancel flag already set, and the call after it
        flag = C.c_int(1)
        assert L.rr_shade_rays_device(h, C.byref(cfg), po, pd, 4, 1, None, p8, None, C.byref(flag)) == -6
        torch.cuda.synchronize()
        assert (out5.cpu().numpy().view(np.uint32) == SENTINEL).all() and (out8.cpu().numpy().view(np.uint32) == SENTINEL).all()
        # from on_pass of the same scene: refused, as every other call there
        seen = []

        def on_pass(frame, done, total):
            seen.append(L.rr_trace_rays_device(h, po, pd, 4, 1, p5, None))
            seen.append(L.rr_trace_shadow_rays_device(h, po, pd, None, 4, 1, p5, None))
            seen.append(L.rr_shade_rays_device(h, C.byref(cfg), po, pd, 4, 1, None, p8, None, None))
            return False
        ds.render_progressive(camera_for(_scene("per_ray_14"), 32, 24).c_struct(), make_config(samples=4, seed=1), on_pass, min_passes=2)
        assert seen and all(code == -1 for code in seen)
        # and the handle answers afterwards
        _same(dev_trace(ds, o, d, 1), host_trace(hip, ds, o, d, 1), "after the refused calls")
        _same(dev_shade(ds, cfg, o, d, 4, 1, None), host_shade(hip, ds, cfg, o, d, 4, 1, None), "after the cancelled call")
