"""rr_accumulate_split_records on the device against the numpy yardstick rustray_amd/temporal.py: accumulate_split_records, every output
word equal.

1: the hand-made split frames of tests/temporal_split_cases.py, clean and with finiteness broken on purpose, at 1x1, 3x2, 33x9 (one pixel
past a 32x8 tile both ways), 37x19 and 130x70: with and without halves and motion, the first frame, snap 0, in place (all four pairs),
sentinels behind all six outputs, absent outputs untouched, the inputs unchanged, behind its producer on a non-null stream; the records,
halves, length and bytes against rr_accumulate_records_device; 2: the host form, the bytes, refusals that launch nothing; 3: end to end on
spheres_room through Raytracing.render_temporal_split -- a static camera over six frames, a moved item; the ordering of the split and the
mean-albedo arm on item 21's checkered floor.

The diffuse words are compared bitwise: the header rules out a generated NaN there.  The only NaN allowance is the one
tests/test_gpu_temporal.py makes for records and halves."""
import ctypes as C

import numpy as np
import pytest

from rustray_amd import denoise
from rustray_amd.temporal import AccumulateParams, accumulate_split_records, previous_view
from tests.denoise_cases import F
from tests.helpers import camera_for
from tests.temporal_cases import frame_params
from tests.temporal_device import check_words as _check, device_call
from tests.temporal_split_cases import split_frame, split_frame_odd
from tests.test_gpu_pixel_parts import SENTINEL, _cfg
from tests.test_gpu_shade_rays import _scene

pytestmark = pytest.mark.gpu

_want = {}
KINDS = {"clean": split_frame, "odd": split_frame_odd}
KEYS = ("records", "halves", "diffuse", "diffuse_halves", "history", "history_halves", "history_diffuse", "history_diffuse_halves", "history_length", "motion")
OUTS = ("out", "halves_out", "diffuse_out", "diffuse_halves_out", "length_out", "rgba")
SIZES = ((1, 1), (3, 2), (33, 9), (37, 19), (130, 70))
COMBOS = ((True, True, False), (True, False, False), (False, True, False), (False, False, False), (True, False, True), (False, False, True))


def _inputs(case, use_halves, use_motion, first):
    hist = lambda k, on=True: case[k] if on and not first else None
    return dict(records=case["records"], halves=case["halves"] if use_halves else None, diffuse=case["diffuse"],
                diffuse_halves=case["diffuse_halves"] if use_halves else None, history=hist("history"), history_halves=hist("history_halves", use_halves),
                history_diffuse=hist("history_diffuse"), history_diffuse_halves=hist("history_diffuse_halves", use_halves),
                history_length=hist("history_length"), motion=case["motion"] if use_motion else None)


def _yardstick(kind, W, H, use_halves, use_motion, first, snap=1 / 64):
    """The yardstick's answer for the case, computed once and left unchanged."""
    key = (kind, W, H, use_halves, use_motion, first, snap)
    if key not in _want:
        case = KINDS[kind](W, H)
        a = _inputs(case, use_halves, use_motion, first)
        _want[key] = accumulate_split_records(*(a[k] for k in KEYS), case["cam"], frame_params(case, snap=snap))
    return _want[key]


@pytest.fixture(scope="module")
def small_scene(hip):
    with hip.DeviceScene(_scene("spheres_room"), 0) as ds:      # any small scene gives the handle
        yield ds


def _device_call(ds, kind, W, H, use_halves, use_motion, first, snap=1 / 64, in_place=False, rgba8=False, stream=None, produce=False, plain=False):
    """One rr_accumulate_split_records_device call on the case through tests/temporal_device.py: sentinels behind every output, the inputs
    checked to be what they were -> dict(records, halves, diffuse, diffuse_halves, length [, rgba]) as numpy words.  in_place: over the
    four current arrays.  plain: rr_accumulate_records_device on the same buffers instead, the diffuse outputs untouched."""
    case = KINDS[kind](W, H)
    return device_call(ds, "plain" if plain else "split", case["cam"].c_struct(), frame_params(case, snap=snap), _inputs(case, use_halves, use_motion, first),
                       in_place=("records", "halves", "diffuse", "diffuse_halves") if in_place else (), rgba8=rgba8, stream=stream, produce=produce)


def _held_share(want, case):
    kept = want["length"] > 1
    same = lambda a, b: (np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all(-1)
    layers = [(want["diffuse"], case["diffuse"])]
    if want["diffuse_halves"] is not None:
        layers += [(want["diffuse_halves"][:, h], case["diffuse_halves"][:, h]) for h in (0, 1)]
    return [float((same(g, c) & kept).sum() / max(int(kept.sum()), 1)) for g, c in layers]


# ---- 1: hand-made frames against the yardstick -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("clean", "odd"))
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("use_halves,use_motion,first", COMBOS)
def test_every_word_equals_the_yardstick(small_scene, kind, W, H, use_halves, use_motion, first):
    want = _yardstick(kind, W, H, use_halves, use_motion, first)
    if not first and W * H >= 33 * 9:
        assert 0.1 < (want["length"] > 1).mean() < 0.9        # the case exercises both paths (the two tiny frames keep no pixel)
        if kind == "odd":
            # a condition on the inputs: the restart rule is exercised, and it does not hide the blend
            shares = _held_share(want, KINDS[kind](W, H))
            assert all(0 < s < 0.1 for s in shares), shares
    _check(_device_call(small_scene, kind, W, H, use_halves, use_motion, first), want, f"{kind} {W}x{H} halves={use_halves} motion={use_motion} first={first}")


@pytest.mark.parametrize("kind", ("clean", "odd"))
@pytest.mark.parametrize("W,H", ((33, 9), (37, 19), (130, 70)))
def test_without_snap_and_in_place(small_scene, kind, W, H):
    _check(_device_call(small_scene, kind, W, H, True, True, False, snap=0.0), _yardstick(kind, W, H, True, True, False, snap=0.0), f"{W}x{H} snap 0")
    _check(_device_call(small_scene, kind, W, H, True, True, False, in_place=True), _yardstick(kind, W, H, True, True, False), f"{W}x{H} in place")
    _check(_device_call(small_scene, kind, W, H, False, False, False, in_place=True), _yardstick(kind, W, H, False, False, False), f"{W}x{H} in place, one layer")
    _check(_device_call(small_scene, kind, W, H, True, False, True, in_place=True), _yardstick(kind, W, H, True, False, True), f"{W}x{H} in place, first frame")


@pytest.mark.parametrize("kind", ("clean", "odd"))
@pytest.mark.parametrize("W,H", SIZES)
def test_records_halves_length_and_bytes_are_those_of_accumulate_records(small_scene, kind, W, H):
    """Identity 1 on the device: whatever the diffuse holds."""
    for use_halves, use_motion, first in ((True, True, False), (False, False, False), (True, False, True)):
        split = _device_call(small_scene, kind, W, H, use_halves, use_motion, first, rgba8=True)
        plain = _device_call(small_scene, kind, W, H, use_halves, use_motion, first, rgba8=True, plain=True)
        _check(split, plain, f"{kind} {W}x{H} against rr_accumulate_records_device", diffuse=False)
        assert np.array_equal(split["length"], plain["length"]) and np.array_equal(split["rgba"], plain["rgba"])


def test_after_its_producer_on_a_non_null_stream(small_scene):
    import torch
    st = torch.cuda.Stream()
    _check(_device_call(small_scene, "odd", 130, 70, True, True, False, stream=st, produce=True), _yardstick("odd", 130, 70, True, True, False), "behind its producer")
    _check(_device_call(small_scene, "clean", 37, 19, True, False, False, stream=st, produce=True, in_place=True), _yardstick("clean", 37, 19, True, False, False),
           "behind its producer, in place")


# ---- 2: the host form, the bytes, refusals ------------------------------------------------------------------------------------------
def test_device_form_equals_host_form_and_the_bytes(small_scene):
    W, H = 130, 70
    case = split_frame_odd(W, H)
    a = _inputs(case, True, True, False)
    prm = frame_params(case)
    cam = case["cam"].c_struct()
    host = small_scene.accumulate_split(cam, *(a[k] for k in KEYS), prm, rgba8=True)
    dev = _device_call(small_scene, "odd", W, H, True, True, False, rgba8=True)
    for k in ("records", "halves", "diffuse", "diffuse_halves", "length"):
        assert np.array_equal(np.ascontiguousarray(host[k]).view(np.uint32).reshape(-1), dev[k].reshape(-1)), k
    assert np.array_equal(host["rgba"], dev["rgba"])
    _check(host, _yardstick("odd", W, H, True, True, False), "host form")
    assert np.array_equal(host["rgba"], denoise.frame_bytes_linear(host["records"][:, 0:3]))
    one = small_scene.accumulate_split(cam, a["records"], None, a["diffuse"], None, a["history"], None, a["history_diffuse"], None, a["history_length"], None, prm,
                                       in_place=True)
    _check(one, _yardstick("odd", W, H, False, False, False), "host form, one layer, in place")
    first = small_scene.accumulate_split(cam, a["records"], a["halves"], a["diffuse"], a["diffuse_halves"], params=prm)
    _check(first, _yardstick("odd", W, H, True, False, True), "host form, first frame")


def test_refusals_launch_nothing(hip):
    import torch
    L = hip.lib()
    W, H = 37, 19
    n = W * H
    case = split_frame(W, H)
    a = _inputs(case, True, True, False)
    names = {k: (k + "_dev").encode() for k in KEYS}
    names.update(out=b"out_dev", halves_out=b"halves_out_dev", diffuse_out=b"diffuse_out_dev", diffuse_halves_out=b"diffuse_halves_out_dev",
                 length_out=b"length_out_dev", rgba=b"rgba8_out_dev")
    words = dict(out=8 * n, halves_out=16 * n, diffuse_out=3 * n, diffuse_halves_out=6 * n, length_out=n, rgba=n)
    fs = _scene("spheres_room")
    cam50, cfg = camera_for(fs, 50, 38).c_struct(), _cfg("plain")
    with hip.DeviceScene(fs, 0) as ds:
        before = ds.render(cam50, cfg, aux=True)
        stats = ds.stats()
        dev = {k: torch.from_numpy(np.ascontiguousarray(v).copy()).cuda() for k, v in a.items()}
        dev.update({k: torch.full((w + 4,), SENTINEL, dtype=torch.int32, device="cuda") for k, w in words.items()})
        torch.cuda.synchronize()
        host = {k: np.ascontiguousarray(v).copy() for k, v in a.items()}
        host.update({k: np.zeros(w, F) for k, w in words.items()})
        prm, cam = hip.accumulate_params(frame_params(case)), case["cam"].c_struct()
        order = KEYS + OUTS

        def call(p):
            return L.rr_accumulate_split_records_device(ds._h, C.byref(cam), C.byref(prm), *(C.c_void_p(p[k]) if p[k] else None for k in order), None)

        good = {k: dev[k].data_ptr() for k in order}
        for key in order:                                               # a pageable pointer, refused by name
            rc = call(dict(good, **{key: host[key].ctypes.data}))
            assert rc == -1 and names[key] in L.rr_last_error(), (key, rc, L.rr_last_error())
        for key in order:                                               # misalignment
            rc = call(dict(good, **{key: good[key] + (4 if key in ("records", "halves", "history", "history_halves", "out", "halves_out") else 2)}))
            assert rc == -1 and b"aligned" in L.rr_last_error(), (key, rc, L.rr_last_error())
        assert call(dict(good, history=good["out"])) == -1 and b"out overlaps history" in L.rr_last_error()
        assert call(dict(good, history_diffuse=good["diffuse_out"])) == -1 and b"diffuse_out overlaps history_diffuse" in L.rr_last_error()
        assert call(dict(good, diffuse_halves=good["diffuse_out"])) == -1 and b"diffuse_out overlaps diffuse_halves" in L.rr_last_error()
        assert call(dict(good, diffuse_out=None)) == -1 and b"diffuse_out is NULL" in L.rr_last_error()
        assert call(dict(good, diffuse_halves_out=None)) == -1 and b"diffuse_halves_out is required" in L.rr_last_error()
        assert call(dict(good, history_diffuse=None)) == -1 and b"history_diffuse is required" in L.rr_last_error()
        assert call(dict(good, history_diffuse_halves=None)) == -1 and b"history_diffuse_halves is required" in L.rr_last_error()
        assert call(dict(good, history_length=None)) == -1 and b"history and history_length" in L.rr_last_error()
        torch.cuda.synchronize()
        for k in OUTS:
            assert (dev[k].cpu().numpy().view(np.uint32) == SENTINEL).all(), k
        assert ds.stats() == stats
        after = ds.render(cam50, cfg, aux=True)
        for k in ("rgba", "normal", "depth", "object_id"):
            assert np.array_equal(before[k], after[k], equal_nan=True), k
        assert call(good) == 0                                          # and the same pointers, all good, are taken
        torch.cuda.synchronize()
        for k, w in words.items():
            got = dev[k].cpu().numpy().view(np.uint32)
            assert (got[:w] != SENTINEL).any() and (got[w:] == SENTINEL).all(), k


# ---- 3: end to end ------------------------------------------------------------------------------------------------------------------
def _np(t):
    return t.cpu().numpy().view(np.uint32)


def _same_frame(got, hist, want, base_records, base_halves, base, what):
    """one frame of render_temporal_split against the chain's arrays, bit for bit"""
    pairs = (("noisy", base_records), ("halves", base_halves), ("diffuse", base["diffuse"]), ("diffuse_halves", base["diffuse_halves"]),
             ("accumulated", hist["records"]), ("accumulated_halves", hist["halves"]), ("accumulated_diffuse", hist["diffuse"]),
             ("accumulated_diffuse_halves", hist["diffuse_halves"]), ("length", hist["length"]), ("records", want["records"]))
    for key, ref in pairs:
        g, w = _np(got[key]).reshape(-1), np.ascontiguousarray(ref, F).view(np.uint32).reshape(-1)
        assert np.array_equal(g, w), (what, key, int((g != w).sum()))


def test_a_static_camera_over_six_frames(hip):
    """spheres_room, 50x38, 6 frames of 4 samples with 6 seeds: render_temporal_split (four calls on one stream, no host trip) equals
    render_pixel_split -> the yardstick -> mean_albedo -> atrous_denoise_split frame by frame, bit for bit; every pixel with a surface
    under it reaches length 6; the diffuse part is there and is not the colour."""
    import torch
    from rustray_amd.denoise import atrous_denoise_split
    from rustray_amd.renderer import Raytracing, TemporalState, _pack_records
    W, H = 50, 38
    fs = _scene("spheres_room")
    camera = camera_for(fs, W, H)
    rt = Raytracing(fs, camera, 0)
    try:
        rt.config = _cfg("plain", samples=4)
        state = TemporalState()
        hist = dict(records=None, halves=None, diffuse=None, diffuse_halves=None, length=None)
        view = previous_view(camera)
        albedo = rt.mean_albedo(samples=4)
        for k in range(6):
            got = rt.render_temporal_split(state, samples=4, seed=100 + k, rgba8=True)
            torch.cuda.synchronize()
            rt.config.seed = 100 + k
            base = rt.render_pixel_split()
            records, halves = _pack_records(base), _pack_records(base["parts"])
            hist = accumulate_split_records(records, halves, base["diffuse"], base["diffuse_halves"], hist["records"], hist["halves"], hist["diffuse"],
                                            hist["diffuse_halves"], hist["length"], None, camera, AccumulateParams(prev_world_to_clip=view[0], prev_eye=view[1]))
            want = atrous_denoise_split(hist["records"], hist["halves"], hist["diffuse"], hist["diffuse_halves"], albedo, W, H)
            _same_frame(got, hist, want, records, halves, base, f"frame {k}")
            assert np.array_equal(_np(got["albedo"]), albedo.view(np.uint32))
            assert np.array_equal(got["rgba"].cpu().numpy(), denoise.frame_bytes_linear(want["records"][:, 0:3])), k
        assert state.frames == 6 and state.history()["diffuse"] is not None
        fin = np.isfinite(hist["records"][:, 0:3]).all(-1)
        surface = fin & np.isfinite(hist["records"][:, 3]) & np.isfinite(hist["records"][:, 4:7]).all(-1)
        assert surface.sum() > W * H // 2 and (hist["length"][surface] == 6).all() and (hist["length"][fin & ~surface] == 1).all()
        d, c = hist["diffuse"], hist["records"][:, 0:3]
        lit = (d > 0).any(-1)
        print(f"{int(surface.sum())} of {W * H} pixels show a surface, {int(lit.sum())} hold direct diffuse light; mean diffuse {float(d[fin].mean()):.4f}, mean colour {float(c[fin].mean()):.4f}")
        assert lit.sum() > W * H // 4 and (d[surface] != c[surface]).any(-1).mean() > 0.5
        # a state of the plain pipeline met by the split one starts anew, and the other way round
        plain = TemporalState()
        rt.render_temporal(plain, samples=4, seed=1)
        again = rt.render_temporal_split(plain, samples=4, seed=2)
        torch.cuda.synchronize()
        assert plain.frames == 1 and set(np.unique(again["length"].cpu().numpy())) <= {0.0, 1.0}
        back = rt.render_temporal(plain, samples=4, seed=3)
        torch.cuda.synchronize()
        assert plain.frames == 2 and (back["length"].cpu().numpy()[surface] == 2).all()
    finally:
        rt.device_scene.close()


def test_a_moved_item_between_two_frames(hip):
    """spheres_room, 50x38, a static camera, two frames; between them the sphere of id 42 is translated by about two pixels through
    apply_scene.  render_temporal_split(track_items=True) -- five calls on one stream -- equals the chain with motion_records, bit for
    bit, and the share of the sphere's pixels at length 2 is render_temporal(track_items=True)'s for the same frames: the length plane is
    shared."""
    import math
    import torch
    from rustray_amd.denoise import atrous_denoise_split
    from rustray_amd.renderer import Raytracing, TemporalState, _pack_records
    from rustray_amd.temporal import motion_records
    from tests.helpers import item_transforms, with_transforms
    W, H = 50, 38
    fs = _scene("spheres_room")
    camera = camera_for(fs, W, H)
    rt = Raytracing(fs, camera, 0)
    try:
        rt.config = _cfg("plain", samples=4)
        state, plain_state = TemporalState(), TemporalState()
        view = previous_view(camera)
        prm = AccumulateParams(prev_world_to_clip=view[0], prev_eye=view[1])

        def frame(seed):
            got = rt.render_temporal_split(state, samples=4, seed=seed, track_items=True)
            plain = rt.render_temporal(plain_state, samples=4, seed=seed, track_items=True)
            torch.cuda.synchronize()
            rt.config.seed = seed
            base = rt.render_pixel_split()
            return got, plain, base, _pack_records(base), _pack_records(base["parts"])

        got, plain, b1, r1, h1 = frame(100)
        assert got["motion"] is None
        first = accumulate_split_records(r1, h1, b1["diffuse"], b1["diffuse_halves"], None, None, None, None, None, None, camera, prm)
        item = next(i for i, it in enumerate(fs.items) if it.id == 42)
        ident = np.uint32(42)
        ids1 = r1[:, 7].view(np.uint32)
        surface = np.isfinite(r1[:, 3]) & np.isfinite(r1[:, 4:7]).all(-1)
        assert ((ids1 == ident) & surface).sum() >= 50
        d, up = np.asarray(camera.dir, np.float64), np.asarray(camera.up, np.float64)
        right = np.cross(d, up) / np.linalg.norm(np.cross(d, up))
        depth = float(np.median(r1[(ids1 == ident) & surface, 3])) + 1.0
        step = 2.0 * depth * 2.0 * math.tan(camera.fov / 2.0) / H
        t, ti = item_transforms(fs)
        move, back = np.eye(4), np.eye(4)
        move[:3, 3], back[:3, 3] = right * step, -right * step
        old = t[item].copy()
        t[item], ti[item] = (move @ t[item].astype(np.float64)).astype(F), (ti[item].astype(np.float64) @ back).astype(F)
        assert rt.apply_scene(with_transforms(_scene("spheres_room"), t, ti)) == ["update_transforms"]

        got, plain, b2, r2, h2 = frame(101)
        albedo = rt.mean_albedo(samples=4)
        motion, _ = motion_records(r2, camera, [ident], old[None], ti[item][None])
        hist = accumulate_split_records(r2, h2, b2["diffuse"], b2["diffuse_halves"], first["records"], first["halves"], first["diffuse"], first["diffuse_halves"],
                                        first["length"], motion, camera, prm)
        want = atrous_denoise_split(hist["records"], hist["halves"], hist["diffuse"], hist["diffuse_halves"], albedo, W, H)
        assert np.array_equal(_np(got["motion"]), motion.view(np.uint32))
        _same_frame(got, hist, want, r2, h2, b2, "the moved frame")
        assert state.frames == 2
        on_sphere = (r2[:, 7].view(np.uint32) == ident) & np.isfinite(r2[:, 3]) & np.isfinite(r2[:, 4:7]).all(-1)
        share = float((hist["length"][on_sphere] == 2).mean())
        share_plain = float((plain["length"].cpu().numpy()[on_sphere] == 2).mean())
        print(f"id 42: {int(on_sphere.sum())} pixels; length == 2 on {share:.3f} of them, {share_plain:.3f} through render_temporal")
        assert on_sphere.sum() >= 50 and share == share_plain and share > 0.5
        assert np.array_equal(_np(got["length"]), _np(plain["length"]))
        assert (hist["diffuse"][on_sphere & (hist["length"] == 2)] != b2["diffuse"][on_sphere & (hist["length"] == 2)]).any()
    finally:
        rt.device_scene.close()


def test_the_other_temporal_pipelines_still_refuse_the_diffuse_arm(hip):
    from rustray_amd import renderer
    from rustray_amd.renderer import Raytracing, TemporalState
    fs = _scene("spheres_room")
    camera = camera_for(fs, 50, 38)
    rt = Raytracing(fs, camera, 0)
    try:
        rt.config = _cfg("plain", samples=4)
        state = TemporalState()
        with pytest.raises(ValueError, match="render_temporal_split"):
            rt.render_temporal(state, samples=4, albedo="diffuse")
        with pytest.raises(ValueError, match="render_temporal_split"):
            renderer.render_temporal_torch(rt.device_scene, camera.c_struct(), rt.config, state, albedo="diffuse")
        assert state.frames == 0
    finally:
        rt.device_scene.close()


def test_quality_on_a_checkered_floor_over_six_frames(hip):
    """Item 21's floor and protocol (50x38, 8 samples a frame in two halves, truth at 512 samples, RMSE of linear colour over the floor's
    853 pixels), a static view: render_temporal(albedo="mean") against render_temporal_split at frame 1 and frame 6; every figure is
    printed.  Asserted: the split arm is below the mean-albedo arm at both frames.  Measured on one MI355X over three seed sets (DESIGN.md
    section 8 item 23): 0.0484 - 0.0492 against 0.1071 - 0.1079, a margin of 0.058 where the seed sets differ by 0.0009 at most.  That
    frame 6 is better than frame 1 is NOT asserted: on this floor it is not, in any arm (the error barely depends on the seed)."""
    import torch
    from rustray_amd.renderer import Raytracing, TemporalState
    from tests.test_gpu_denoise_albedo import H, W, _cfg as _floor_cfg, _checkered_floor
    fs = _checkered_floor()
    camera = camera_for(fs, W, H)
    rt = Raytracing(fs, camera, 0)
    try:
        rt.config = _floor_cfg(samples=512)
        truth = rt.render_pixels()["color"].astype(np.float64)
        surf = rt.surface_pixels()
        floor = (surf["hit"] == 1) & (surf["object_id"] == 3)
        assert floor.sum() > W * H // 4
        rt.config = _floor_cfg(samples=8)
        rmse = lambda t: float(np.sqrt(((t.cpu().numpy()[floor, 0:3].astype(np.float64) - truth[floor]) ** 2).mean()))
        mean_state, split_state = TemporalState(), TemporalState()
        for k in range(6):
            mean = rt.render_temporal(mean_state, samples=8, seed=100 + k, albedo="mean")
            split = rt.render_temporal_split(split_state, samples=8, seed=100 + k)
            torch.cuda.synchronize()
            if k in (0, 5):
                a, b = rmse(mean["records"]), rmse(split["records"])
                print(f"checkered floor, frame {k + 1}, {int(floor.sum())} pixels, RMSE against 512 samples: mean albedo {a:.6f}, split {b:.6f}")
                assert np.isfinite([a, b]).all() and b < a, (k, a, b)
        length = split["length"].cpu().numpy()
        print(f"floor pixels at length 6 after six frames: {float((length[floor] == 6).mean()):.3f}")
        assert np.array_equal(length, mean["length"].cpu().numpy()) and length[floor].max() == 6      # the two pipelines share the length plane
    finally:
        rt.device_scene.close()
