"""rr_accumulate_clamped_split_records on the device against the numpy yardstick rustray_amd/temporal.py:
accumulate_clamped_split_records, every output word equal.

1: the hand-made frames of tests/temporal_clamp_split_cases.py, clean and odd, at 1x1 and 3x2 (the windows are larger than the frame),
32x8 (exactly one tile: the halo is all outside), 33x9 (one pixel past a tile both ways), 64x16 (a halo that reads the interior of the
next tile both ways), 37x19 and 130x70: both radii, sigma_scale 1 and 2, with and without halves and motion, the first frame; sentinels
behind all six outputs, absent outputs untouched, inputs unchanged, halves and diffuse halves in place, behind its producer on a non-null
stream; 2: the host form, the bytes, refusals that launch nothing, the colour side against rr_accumulate_clamped_records_device and a
history of the frame's own layers against rr_accumulate_split_records_device; 3: end to end on spheres_room through
Raytracing.render_temporal_split_clamped with a light edit before frame 5.

The diffuse words are compared bitwise: the header rules out a generated NaN there.  The only NaN allowance is the one
tests/test_gpu_temporal.py makes for records and halves."""
import copy
import ctypes as C

import numpy as np
import pytest

from rustray_amd import denoise
from rustray_amd.temporal import AccumulateParams, HistoryClampParams, accumulate_clamped_split_records, previous_view
from tests.denoise_cases import F
from tests.helpers import camera_for
from tests.temporal_cases import frame_params
from tests.temporal_device import check_words as _check, device_call
from tests.temporal_clamp_split_cases import KEYS, KINDS, clamp_split_frame, inputs, own_colour_split_frame
from tests.test_gpu_pixel_parts import SENTINEL, _cfg
from tests.test_gpu_shade_rays import _scene

pytestmark = pytest.mark.gpu

_want = {}
OUTS = ("out", "halves_out", "diffuse_out", "diffuse_halves_out", "length_out", "rgba")
SIZES = ((1, 1), (3, 2), (32, 8), (33, 9), (64, 16), (37, 19), (130, 70))
COMBOS = ((True, True, False), (True, False, False), (False, True, False), (False, False, False), (True, False, True), (False, False, True))
LAYERS = ("records", "halves", "diffuse", "diffuse_halves", "length")


def _yardstick(kind, W, H, use_halves, use_motion, first, clamp, snap=1 / 64):
    """The yardstick's answer for the case, computed once and left unchanged."""
    key = (kind, W, H, use_halves, use_motion, first, clamp, snap)
    if key not in _want:
        case = KINDS[kind](W, H)
        _want[key] = accumulate_clamped_split_records(*inputs(case, use_halves, use_motion, first), case["cam"], frame_params(case, snap=snap),
                                                      HistoryClampParams(*clamp))
    return _want[key]


@pytest.fixture(scope="module")
def small_scene(hip):
    with hip.DeviceScene(_scene("spheres_room"), 0) as ds:      # any small scene gives the handle
        yield ds


def _device_call(ds, case, prm, a, clamp, halves_in_place=False, rgba8=False, stream=None, produce=False, call="clamped_split"):
    """One rr_accumulate_clamped_split_records_device call on the arrays `a` (inputs(...)) through tests/temporal_device.py: sentinels
    behind every output, the inputs checked to be what they were -> dict(records, halves, diffuse, diffuse_halves, length [, rgba]) as
    numpy words.  call="clamped": rr_accumulate_clamped_records_device on the colour buffers instead, the diffuse outputs untouched;
    call="split": rr_accumulate_split_records_device on all of them."""
    return device_call(ds, call, case["cam"].c_struct(), prm, dict(zip(KEYS, a)), clamp=clamp, in_place=("halves", "diffuse_halves") if halves_in_place else (),
                       rgba8=rgba8, stream=stream, produce=produce)


def _case_call(ds, kind, W, H, use_halves, use_motion, first, clamp, snap=1 / 64, **kw):
    case = KINDS[kind](W, H)
    return _device_call(ds, case, frame_params(case, snap=snap), inputs(case, use_halves, use_motion, first), clamp, **kw)


# ---- 1: hand-made frames against the yardstick -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("clean", "odd"))
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("clamp", ((1, 1.0), (2, 1.0), (1, 2.0), (2, 2.0)))
def test_every_word_equals_the_yardstick(small_scene, kind, W, H, clamp):
    for use_halves, use_motion, first in COMBOS:
        want = _yardstick(kind, W, H, use_halves, use_motion, first, clamp)
        if not first and W * H >= 33 * 9 and kind == "clean" and clamp[1] == 1.0:
            kept = want["length"] > 1          # the case exercises every path: kept or not, each kind of layer moved or not
            assert 0.1 < kept.mean() < 0.9 and 0.05 < want["clamped"][:, 0].sum() / max(kept.sum(), 1) and 0.05 < want["diffuse_clamped"][:, 0].sum() / max(kept.sum(), 1)
        _check(_case_call(small_scene, kind, W, H, use_halves, use_motion, first, clamp), want,
               f"{kind} {W}x{H} clamp={clamp} halves={use_halves} motion={use_motion} first={first}")


@pytest.mark.parametrize("kind", ("clean", "odd"))
@pytest.mark.parametrize("W,H", ((33, 9), (64, 16), (130, 70)))
def test_without_snap_at_the_edges_of_sigma_scale_and_halves_in_place(small_scene, kind, W, H):
    _check(_case_call(small_scene, kind, W, H, True, True, False, (2, 1.0), snap=0.0), _yardstick(kind, W, H, True, True, False, (2, 1.0), snap=0.0), f"{W}x{H} snap 0")
    for clamp in ((1, 0.0), (2, 65536.0), (1, 0.5)):
        _check(_case_call(small_scene, kind, W, H, True, True, False, clamp), _yardstick(kind, W, H, True, True, False, clamp), f"{W}x{H} clamp={clamp}")
    _check(_case_call(small_scene, kind, W, H, True, True, False, (1, 1.0), halves_in_place=True), _yardstick(kind, W, H, True, True, False, (1, 1.0)),
           f"{W}x{H} halves and diffuse halves in place")
    _check(_case_call(small_scene, kind, W, H, True, False, True, (2, 2.0), halves_in_place=True), _yardstick(kind, W, H, True, False, True, (2, 2.0)),
           f"{W}x{H} halves and diffuse halves in place, first frame")


def test_after_its_producer_on_a_non_null_stream(small_scene):
    import torch
    st = torch.cuda.Stream()
    _check(_case_call(small_scene, "odd", 130, 70, True, True, False, (2, 1.0), stream=st, produce=True), _yardstick("odd", 130, 70, True, True, False, (2, 1.0)),
           "behind its producer")
    _check(_case_call(small_scene, "clean", 37, 19, True, False, False, (1, 1.0), stream=st, produce=True, halves_in_place=True),
           _yardstick("clean", 37, 19, True, False, False, (1, 1.0)), "behind its producer, halves in place")


# ---- 2: the host form, the bytes, refusals, the two older calls ---------------------------------------------------------------------
def test_device_form_equals_host_form_and_the_bytes(small_scene):
    W, H = 130, 70
    case = KINDS["odd"](W, H)
    prm, clamp = frame_params(case), HistoryClampParams(2, 1.0)
    cam = case["cam"].c_struct()
    a = inputs(case, True, True, False)
    host = small_scene.accumulate_clamped_split(cam, *a, prm, clamp, rgba8=True)
    dev = _case_call(small_scene, "odd", W, H, True, True, False, (2, 1.0), rgba8=True)
    for k in LAYERS:
        assert np.array_equal(np.ascontiguousarray(host[k]).view(np.uint32).reshape(-1), dev[k].reshape(-1)), k
    assert np.array_equal(host["rgba"], dev["rgba"])
    _check(host, _yardstick("odd", W, H, True, True, False, (2, 1.0)), "host form")
    assert np.array_equal(host["rgba"], denoise.frame_bytes_linear(host["records"][:, 0:3]))
    a1 = inputs(case, False, False, False)
    one = small_scene.accumulate_clamped_split(cam, *a1, prm, HistoryClampParams(1, 2.0))
    _check(one, _yardstick("odd", W, H, False, False, False, (1, 2.0)), "host form, one layer")
    first = small_scene.accumulate_clamped_split(cam, a[0], a[1], a[2], a[3], params=prm, clamp=clamp, halves_in_place=True)
    _check(first, _yardstick("odd", W, H, True, False, True, (2, 1.0)), "host form, first frame, halves in place")
    dflt = small_scene.accumulate_clamped_split(cam, *a, prm)
    d = HistoryClampParams()
    _check(dflt, _yardstick("odd", W, H, True, True, False, (d.radius, d.sigma_scale)), "host form, the library's default clamp")


def test_refusals_launch_nothing(hip):
    import torch
    L = hip.lib()
    W, H = 37, 19
    n = W * H
    case = clamp_split_frame(W, H)
    a = dict(zip(KEYS, inputs(case, True, True, False)))
    names = {k: (k + "_dev").encode() for k in KEYS}
    names.update(out=b"out_dev", halves_out=b"halves_out_dev", diffuse_out=b"diffuse_out_dev", diffuse_halves_out=b"diffuse_halves_out_dev",
                 length_out=b"length_out_dev", rgba=b"rgba8_out_dev")
    words = dict(out=8 * n, halves_out=16 * n, diffuse_out=3 * n, diffuse_halves_out=6 * n, length_out=n, rgba=n)
    fs = _scene("spheres_room")
    cam50, cfg = camera_for(fs, 50, 38).c_struct(), _cfg("plain")
    fn = b"rr_accumulate_clamped_split_records_device"
    with hip.DeviceScene(fs, 0) as ds:
        before = ds.render(cam50, cfg, aux=True)
        stats = ds.stats()
        dev = {k: torch.from_numpy(np.ascontiguousarray(v).copy()).cuda() for k, v in a.items()}
        dev.update({k: torch.full((w + 4,), SENTINEL, dtype=torch.int32, device="cuda") for k, w in words.items()})
        torch.cuda.synchronize()
        host = {k: np.ascontiguousarray(v).copy() for k, v in a.items()}
        host.update({k: np.zeros(w, F) for k, w in words.items()})
        prm, cam, clamp = hip.accumulate_params(frame_params(case)), case["cam"].c_struct(), hip.history_clamp_default_params()
        order = KEYS + OUTS

        def call(p, k=clamp):
            return L.rr_accumulate_clamped_split_records_device(ds._h, C.byref(cam), C.byref(prm), C.byref(k) if k is not None else None,
                                                                *(C.c_void_p(p[x]) if p[x] else None for x in order), None)

        err = lambda: L.rr_last_error()
        good = {k: dev[k].data_ptr() for k in order}
        for key in order:                                               # a pageable pointer, refused by name
            rc = call(dict(good, **{key: host[key].ctypes.data}))
            assert rc == -1 and names[key] in err() and fn in err(), (key, rc, err())
        for key in order:                                               # misalignment
            rc = call(dict(good, **{key: good[key] + (4 if key in ("records", "halves", "history", "history_halves", "out", "halves_out") else 2)}))
            assert rc == -1 and b"aligned" in err() and fn in err(), (key, rc, err())
        assert call(dict(good, out=good["records"])) == -1 and b"out overlaps records" in err() and b"windows read" in err() and fn in err()
        assert call(dict(good, diffuse_out=good["diffuse"])) == -1 and b"diffuse_out overlaps diffuse " in err() and b"windows read" in err() and fn in err()
        assert call(dict(good, history=good["out"])) == -1 and b"out overlaps history" in err()
        assert call(dict(good, history_diffuse=good["diffuse_out"])) == -1 and b"diffuse_out overlaps history_diffuse" in err()
        assert call(dict(good, diffuse_halves=good["diffuse_out"])) == -1 and b"diffuse_out overlaps diffuse_halves" in err()
        assert call(dict(good, diffuse_out=None)) == -1 and b"diffuse_out is NULL" in err()
        assert call(dict(good, diffuse_halves_out=None)) == -1 and b"diffuse_halves_out is required" in err()
        assert call(dict(good, history_diffuse=None)) == -1 and b"history_diffuse is required" in err()
        assert call(dict(good, history_diffuse_halves=None)) == -1 and b"history_diffuse_halves is required" in err()
        assert call(dict(good, history_length=None)) == -1 and b"history and history_length" in err()
        assert call(good, None) == -1 and b"clamp is NULL" in err() and fn in err()
        for fld, val in (("struct_size", 16), ("radius", 3), ("radius", 0), ("sigma_scale", float("nan")), ("sigma_scale", -1.0), ("sigma_scale", 65537.0)):
            k = hip.history_clamp_default_params()
            setattr(k, fld, val)
            assert call(good, k) == -1 and b"clamp->" + fld.encode() in err() and fn in err(), (fld, val)
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


@pytest.mark.parametrize("kind", ("clean", "odd"))
@pytest.mark.parametrize("W,H", ((3, 2), (33, 9), (130, 70)))
def test_records_halves_length_and_bytes_are_those_of_the_clamped_call(small_scene, kind, W, H):
    """The invariant carried over, on the device: whatever the diffuse holds, out, halves_out, length_out and rgba8_out are
    rr_accumulate_clamped_records_device's bits."""
    case = KINDS[kind](W, H)
    for radius in (1, 2):
        for use_halves, use_motion, first in ((True, True, False), (False, False, False), (True, False, True)):
            a = inputs(case, use_halves, use_motion, first)
            got = _device_call(small_scene, case, frame_params(case), a, (radius, 1.0), rgba8=True)
            colour = _device_call(small_scene, case, frame_params(case), a, (radius, 1.0), rgba8=True, call="clamped")
            for k in ("records", "length", "rgba") + (("halves",) if use_halves else ()):
                assert np.array_equal(got[k], colour[k]), (k, kind, radius, use_halves, first)


@pytest.mark.parametrize("W,H", ((33, 9), (130, 70)))
def test_a_history_of_the_frames_own_layers_is_rr_accumulate_split_records(small_scene, W, H):
    """The history holds the current frame in every layer under the camera's own view, both halves of a pixel hold its record's colour and
    both diffuse halves its diffuse, so every history mean of every layer is a member of the window its box is made from.  A member of m
    values lies within sqrt(m - 1) standard deviations of their mean (2.83 at 3x3, 4.90 at 5x5): at sigma_scale 8 nothing leaves any box,
    and every output word is rr_accumulate_split_records_device's."""
    case, prm = own_colour_split_frame(W, H)
    for radius in (1, 2):
        for use_halves in (True, False):
            a = inputs(case, use_halves, False, False)
            want = accumulate_clamped_split_records(*a, case["cam"], prm, HistoryClampParams(radius, 8.0))
            assert not want["clamped"].any() and not want["diffuse_clamped"].any() and (want["length"] > 1).mean() > 0.5
            got = _device_call(small_scene, case, prm, a, (radius, 8.0), rgba8=True)
            split = _device_call(small_scene, case, prm, a, (radius, 8.0), rgba8=True, call="split")
            for k in ("records", "length", "rgba", "diffuse") + (("halves", "diffuse_halves") if use_halves else ()):
                assert np.array_equal(got[k], split[k]), (k, radius, use_halves)


# ---- 3: end to end ------------------------------------------------------------------------------------------------------------------
W3, H3, FRAMES, EDIT_AT = 50, 38, 8, 4


def _edited(fs):
    """spheres_room under other lights: every light four times as strong and tinted (item 24's edit)"""
    new = copy.deepcopy(fs)
    for light in new.lights:
        light.intensity = light.intensity * 4.0
        light.color = (light.color[0], light.color[1] * 0.5, light.color[2] * 0.25)
    return new


def _np(t):
    return t.cpu().numpy().view(np.uint32)


def test_render_temporal_split_clamped_equals_the_chain(hip):
    """render_temporal_split_clamped(state) equals render_pixel_split -> accumulate_clamped_split_records -> mean_albedo ->
    atrous_denoise_split frame by frame, bit for bit, over the eight frames of item 24's protocol (spheres_room 50x38, 4 samples, the lights
    edited before the fifth frame), for the default clamp and for one given; over those frames more than 100 diffuse-layer clamps are
    counted; a state may pass between the clamped and the unclamped split pipeline; a missing or bad clamp is refused before anything is
    rendered or noted."""
    import torch
    from rustray_amd.denoise import atrous_denoise_split
    from rustray_amd.renderer import Raytracing, TemporalState, _pack_records, render_temporal_split_clamped_torch
    fs = _scene("spheres_room")
    camera = camera_for(fs, W3, H3)
    rt = Raytracing(fs, camera, 0)
    try:
        rt.config = _cfg("plain", samples=4)
        view = previous_view(camera)
        prm = AccumulateParams(prev_world_to_clip=view[0], prev_eye=view[1])
        for clamp, as_params in ((True, HistoryClampParams()), (HistoryClampParams(2, 0.5), HistoryClampParams(2, 0.5))):
            state = TemporalState()
            hist = dict(records=None, halves=None, diffuse=None, diffuse_halves=None, length=None)
            colour_clamps = diffuse_clamps = 0
            for k in range(FRAMES):
                if k == EDIT_AT:
                    assert rt.apply_scene(_edited(_scene("spheres_room"))) == ["update_lights"]
                got = rt.render_temporal_split_clamped(state, samples=4, seed=100 + k, clamp=clamp, rgba8=True)
                torch.cuda.synchronize()
                rt.config.seed = 100 + k
                base = rt.render_pixel_split()
                albedo = rt.mean_albedo(samples=4)
                records, halves = _pack_records(base), _pack_records(base["parts"])
                hist = accumulate_clamped_split_records(records, halves, base["diffuse"], base["diffuse_halves"], hist["records"], hist["halves"], hist["diffuse"],
                                                        hist["diffuse_halves"], hist["length"], None, camera, prm, as_params)
                want = atrous_denoise_split(hist["records"], hist["halves"], hist["diffuse"], hist["diffuse_halves"], albedo, W3, H3)
                pairs = (("noisy", records), ("halves", halves), ("diffuse", base["diffuse"]), ("diffuse_halves", base["diffuse_halves"]),
                         ("accumulated", hist["records"]), ("accumulated_halves", hist["halves"]), ("accumulated_diffuse", hist["diffuse"]),
                         ("accumulated_diffuse_halves", hist["diffuse_halves"]), ("length", hist["length"]), ("records", want["records"]))
                for key, ref in pairs:
                    g, w = _np(got[key]).reshape(-1), np.ascontiguousarray(ref, F).view(np.uint32).reshape(-1)
                    assert np.array_equal(g, w), (clamp, k, key, int((g != w).sum()))
                assert np.array_equal(got["rgba"].cpu().numpy(), denoise.frame_bytes_linear(want["records"][:, 0:3])), k
                colour_clamps += int(hist["clamped"][:, 0].sum())
                diffuse_clamps += int(hist["diffuse_clamped"][:, 0].sum())
            print(f"clamp {as_params}: {colour_clamps} record-layer and {diffuse_clamps} diffuse-layer clamps over {FRAMES} frames")
            assert state.frames == FRAMES and colour_clamps > 100 and diffuse_clamps > 100
            # the unclamped split pipeline takes the state on (the same sets), and hands it back
            on = rt.render_temporal_split(state, samples=4, seed=200)
            back = rt.render_temporal_split_clamped(state, samples=4, seed=201, clamp=clamp)
            torch.cuda.synchronize()
            assert state.frames == FRAMES + 2 and float(on["length"].max()) > 2 and float(back["length"].max()) > 2
            rt.apply_scene(_scene("spheres_room"))
        fresh = TemporalState()
        for bad in (None, False, "yes", 1.5, HistoryClampParams(3, 1.0), HistoryClampParams(1, -1.0)):
            with pytest.raises(ValueError):
                rt.render_temporal_split_clamped(fresh, samples=4, clamp=bad, track_items=True)
            with pytest.raises(ValueError):
                render_temporal_split_clamped_torch(rt.device_scene, camera.c_struct(), rt.config, fresh, clamp=bad)
        assert fresh.frames == 0 and fresh.items is None and fresh.sets == [None, None]
        with pytest.raises(ValueError, match="render_temporal_split_clamped"):
            rt.render_temporal_split(TemporalState(), samples=4, clamp=True)
    finally:
        rt.device_scene.close()


def test_a_moved_item_under_the_clamped_split_pipeline(hip):
    """track_items=True: between two frames one sphere is translated by about two pixels through apply_scene; the motion of the moved item
    is made on the device on the same stream, and the frame equals the chain with motion_records, bit for bit."""
    import math
    import torch
    from rustray_amd.renderer import Raytracing, TemporalState, _pack_records
    from rustray_amd.temporal import motion_records
    from tests.helpers import item_transforms, with_transforms
    fs = _scene("spheres_room")
    camera = camera_for(fs, W3, H3)
    rt = Raytracing(fs, camera, 0)
    try:
        rt.config = _cfg("plain", samples=4)
        state = TemporalState()
        view = previous_view(camera)
        prm = AccumulateParams(prev_world_to_clip=view[0], prev_eye=view[1])

        def frame(seed):
            got = rt.render_temporal_split_clamped(state, samples=4, seed=seed, track_items=True)
            torch.cuda.synchronize()
            rt.config.seed = seed
            base = rt.render_pixel_split()
            return got, base, _pack_records(base), _pack_records(base["parts"])

        got, b1, r1, h1 = frame(100)
        assert got["motion"] is None
        first = accumulate_clamped_split_records(r1, h1, b1["diffuse"], b1["diffuse_halves"], None, None, None, None, None, None, camera, prm)
        item = next(i for i, it in enumerate(fs.items) if it.id == 42)
        ident = np.uint32(42)
        on = (r1[:, 7].view(np.uint32) == ident) & np.isfinite(r1[:, 3]) & np.isfinite(r1[:, 4:7]).all(-1)
        d, up = np.asarray(camera.dir, np.float64), np.asarray(camera.up, np.float64)
        right = np.cross(d, up) / np.linalg.norm(np.cross(d, up))
        step = 2.0 * (float(np.median(r1[on, 3])) + 1.0) * 2.0 * math.tan(camera.fov / 2.0) / H3
        t, ti = item_transforms(fs)
        move, back = np.eye(4), np.eye(4)
        move[:3, 3], back[:3, 3] = right * step, -right * step
        old = t[item].copy()
        t[item], ti[item] = (move @ t[item].astype(np.float64)).astype(F), (ti[item].astype(np.float64) @ back).astype(F)
        assert rt.apply_scene(with_transforms(_scene("spheres_room"), t, ti)) == ["update_transforms"]
        got, b2, r2, h2 = frame(101)
        motion, _ = motion_records(r2, camera, [ident], old[None], ti[item][None])
        hist = accumulate_clamped_split_records(r2, h2, b2["diffuse"], b2["diffuse_halves"], first["records"], first["halves"], first["diffuse"],
                                                first["diffuse_halves"], first["length"], motion, camera, prm)
        assert np.array_equal(_np(got["motion"]), motion.view(np.uint32)) and (motion != 0).any()
        for key, ref in (("accumulated", hist["records"]), ("accumulated_halves", hist["halves"]), ("accumulated_diffuse", hist["diffuse"]),
                         ("accumulated_diffuse_halves", hist["diffuse_halves"]), ("length", hist["length"])):
            assert np.array_equal(_np(got[key]).reshape(-1), np.ascontiguousarray(ref, F).view(np.uint32).reshape(-1)), key
        assert state.frames == 2 and (hist["length"][on] > 1).mean() > 0.3
    finally:
        rt.device_scene.close()


def test_a_light_edit_is_followed_by_the_clamped_split_pipeline(hip):
    """Item 24's protocol (spheres_room 50x38, a static camera, eight frames of 4 samples, every light four times as strong and tinted before
    frame 5), the unclamped split pipeline against render_temporal_split_clamped with the library's defaults, for the seed sets 100..,
    200.. and 300...  The error is the RMSE of the accumulated records over the surface pixels against 512-sample truth under the lights
    of the frame.  Asserted at frames 5 and 6, for every seed set: the clamped error lies below the unclamped one by at least three times
    the largest difference between the seed sets of either arm at that frame.  Every figure is printed."""
    import torch
    from rustray_amd.renderer import Raytracing, TemporalState
    fs = _scene("spheres_room")
    camera = camera_for(fs, W3, H3)
    rt = Raytracing(fs, camera, 0)
    try:
        rt.config = _cfg("plain", samples=512)
        assert rt.apply_scene(_edited(_scene("spheres_room"))) == ["update_lights"]
        truth_new = rt.render_pixels()["color"].astype(np.float64)
        rt.apply_scene(_scene("spheres_room"))
        rt.config = _cfg("plain", samples=4)
        errors = {arm: np.zeros((3, 2)) for arm in ("unclamped", "clamped")}
        surface = None
        for s, seed0 in enumerate((100, 200, 300)):
            states = dict(unclamped=TemporalState(), clamped=TemporalState())
            for k in range(EDIT_AT + 2):
                if k == EDIT_AT:
                    assert rt.apply_scene(_edited(_scene("spheres_room"))) == ["update_lights"]
                for arm, state in states.items():
                    run = rt.render_temporal_split if arm == "unclamped" else rt.render_temporal_split_clamped
                    got = run(state, samples=4, seed=seed0 + k)
                    torch.cuda.synchronize()
                    if surface is None:
                        rec = got["noisy"].cpu().numpy()
                        surface = np.isfinite(rec[:, 0:3]).all(-1) & np.isfinite(rec[:, 3]) & np.isfinite(rec[:, 4:7]).all(-1)
                    if k >= EDIT_AT:
                        acc = got["accumulated"].cpu().numpy()[surface, 0:3].astype(np.float64)
                        errors[arm][s, k - EDIT_AT] = float(np.sqrt(((acc - truth_new[surface]) ** 2).mean()))
            rt.apply_scene(_scene("spheres_room"))
        assert surface.sum() > W3 * H3 // 2
        for j, frame in enumerate((EDIT_AT + 1, EDIT_AT + 2)):
            u, c = errors["unclamped"][:, j], errors["clamped"][:, j]
            spread = max(float(u.max() - u.min()), float(c.max() - c.min()))
            print(f"frame {frame}: RMSE unclamped split {u.round(5).tolist()} clamped split {c.round(5).tolist()} (seeds 100.., 200.., 300..); "
                  f"largest difference between seed sets {spread:.5f}, smallest margin {float((u - c).min()):.5f}")
            assert np.isfinite(u).all() and np.isfinite(c).all() and ((u - c) >= 3 * spread).all() and (c < u).all(), (frame, u, c, spread)
    finally:
        rt.device_scene.close()
