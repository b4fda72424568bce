"""rr_accumulate_records on the device against the numpy yardstick rustray_amd/temporal.py, every output word equal.

1: the hand-made frames and histories of tests/temporal_cases.py at 37x19 and 130x70 (several workgroups both ways, taps across tile
seams): with and without halves and motion, the first frame, in place, sentinels behind every output, the inputs unchanged, behind its
producer on a non-null stream; 2: the host form, the bytes, refusals that launch nothing; 3: end to end on spheres_room -- a static
camera over six frames, a camera yaw; 4: the handle afterwards, an edit behind a call in flight."""
import ctypes as C

import numpy as np
import pytest

from rustray_amd import denoise
from rustray_amd.denoise import atrous_denoise
from rustray_amd.temporal import AccumulateParams, accumulate_records, previous_view
from tests.denoise_cases import F
from tests.helpers import camera_for
from tests.temporal_cases import frame_params, temporal_frame
from tests.temporal_device import check_words as _check, device_call
from tests.test_gpu_pixel_parts import SENTINEL, _cfg
from tests.test_gpu_shade_rays import _scene

pytestmark = pytest.mark.gpu

_want = {}
KEYS = ("records", "halves", "history", "history_halves", "history_length", "motion")


def _inputs(case, use_halves, use_motion, first):
    return dict(records=case["records"], halves=case["halves"] if use_halves else None, history=None if first else case["history"],
                history_halves=case["history_halves"] if use_halves and not first else None, history_length=None if first else case["history_length"],
                motion=case["motion"] if use_motion else None)


def _yardstick(W, H, use_halves, use_motion, first, snap=1 / 64):
    """The yardstick's answer for temporal_frame(W, H), computed once per case and left unchanged."""
    key = (W, H, use_halves, use_motion, first, snap)
    if key not in _want:
        case = temporal_frame(W, H)
        a = _inputs(case, use_halves, use_motion, first)
        _want[key] = accumulate_records(*(a[k] for k in KEYS), case["cam"], frame_params(case, snap=snap))
    return _want[key]


@pytest.fixture(scope="module")
def small_scene(hip):
    with hip.DeviceScene(_scene("spheres_room"), 0) as ds:      # any small scene gives the handle
        yield ds


def _device_call(ds, W, H, use_halves, use_motion, first, snap=1 / 64, in_place=False, rgba8=False, stream=None, produce=False):
    """One rr_accumulate_records_device call on temporal_frame(W, H) through tests/temporal_device.py: sentinels behind every output, the
    inputs checked to be what they were -> dict(records, halves, length [, rgba]) as numpy words.  in_place: over records and halves."""
    case = temporal_frame(W, H)
    return device_call(ds, "plain", case["cam"].c_struct(), frame_params(case, snap=snap), _inputs(case, use_halves, use_motion, first),
                       in_place=("records", "halves") if in_place else (), rgba8=rgba8, stream=stream, produce=produce)


# ---- 1: hand-made frames against the yardstick -------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", ((37, 19), (130, 70)))
@pytest.mark.parametrize("use_halves,use_motion,first", ((True, True, False), (True, False, False), (False, True, False), (False, False, False),
                                                         (True, False, True), (False, False, True)))
def test_every_word_equals_the_yardstick(small_scene, W, H, use_halves, use_motion, first):
    want = _yardstick(W, H, use_halves, use_motion, first)
    if not first:
        assert 0.1 < (want["length"] > 1).mean() < 0.9        # the case exercises both paths
    _check(_device_call(small_scene, W, H, use_halves, use_motion, first), want, f"{W}x{H} halves={use_halves} motion={use_motion} first={first}")


@pytest.mark.parametrize("W,H", ((37, 19), (130, 70)))
def test_without_snap_and_in_place(small_scene, W, H):
    _check(_device_call(small_scene, W, H, True, True, False, snap=0.0), _yardstick(W, H, True, True, False, snap=0.0), f"{W}x{H} snap 0")
    _check(_device_call(small_scene, W, H, True, True, False, in_place=True), _yardstick(W, H, True, True, False), f"{W}x{H} in place")
    _check(_device_call(small_scene, W, H, False, False, False, in_place=True), _yardstick(W, H, False, False, False), f"{W}x{H} in place, one layer")


def test_after_its_producer_on_a_non_null_stream(small_scene):
    import torch
    st = torch.cuda.Stream()
    _check(_device_call(small_scene, 130, 70, True, True, False, stream=st, produce=True), _yardstick(130, 70, True, True, False), "behind its producer")
    _check(_device_call(small_scene, 37, 19, True, False, False, stream=st, produce=True, in_place=True), _yardstick(37, 19, True, False, False),
           "behind its producer, in place")


# ---- 2: the host form, the bytes, refusals ------------------------------------------------------------------------------------------
def test_device_form_equals_host_form_and_the_bytes(small_scene):
    W, H = 130, 70
    case = temporal_frame(W, H)
    a = _inputs(case, True, True, False)
    prm = frame_params(case)
    cam = case["cam"].c_struct()
    host = small_scene.accumulate_records(cam, *(a[k] for k in KEYS), prm, rgba8=True)
    dev = _device_call(small_scene, W, H, True, True, False, rgba8=True)
    for k in ("records", "halves", "length"):
        assert np.array_equal(np.ascontiguousarray(host[k]).view(np.uint32).reshape(-1), dev[k].reshape(-1)), k
    assert np.array_equal(host["rgba"], dev["rgba"])
    _check({k: host[k] for k in ("records", "halves", "length")}, _yardstick(W, H, True, True, False), "host form")
    assert np.array_equal(host["rgba"], denoise.frame_bytes_linear(host["records"][:, 0:3]))
    one = small_scene.accumulate_records(cam, a["records"], None, a["history"], None, a["history_length"], None, prm, in_place=True)
    _check(one, _yardstick(W, H, False, False, False), "host form, one layer, in place")


@pytest.mark.parametrize("gamma", (False, True))
def test_the_bytes_are_render_pixels_bytes(hip, gamma):
    """On the first frame out is the current record, bit for bit: the bytes must be the ones rr_render_pixels wrote for that record."""
    fs = _scene("spheres_room")
    cam = camera_for(fs, 50, 38).c_struct()
    cfg = _cfg("plain", samples=4, gamma_correction=gamma)
    from rustray_amd.renderer import _pack_records
    with hip.DeviceScene(fs, 0) as ds:
        frame = ds.render_pixels(cam, cfg, None, rgba8=True)
        records = _pack_records(frame)
        got = ds.accumulate_records(cam, records, params=AccumulateParams(gamma_correction=gamma), rgba8=True)
    assert np.array_equal(got["records"].view(np.uint32), records.view(np.uint32))
    assert np.array_equal(got["rgba"], frame["rgba"])
    assert np.array_equal(got["rgba"], denoise.frame_bytes_linear(records[:, 0:3])) != gamma


def test_refusals_launch_nothing(small_scene, hip):
    import torch
    L = hip.lib()
    W, H = 37, 19
    n = W * H
    case = temporal_frame(W, H)
    a = _inputs(case, True, True, False)
    names = dict(records=b"records_dev", halves=b"halves_dev", history=b"history_dev", history_halves=b"history_halves_dev", history_length=b"history_length_dev",
                 motion=b"motion_dev", out=b"out_dev", halves_out=b"halves_out_dev", length_out=b"length_out_dev", rgba=b"rgba8_out_dev")
    dev = {k: torch.from_numpy(np.ascontiguousarray(v).copy()).cuda() for k, v in a.items()}
    dev.update(out=torch.full((n + 1, 8), SENTINEL, dtype=torch.int32, device="cuda"), halves_out=torch.full((2 * n + 1, 8), SENTINEL, dtype=torch.int32, device="cuda"),
               length_out=torch.full((n + 1,), SENTINEL, dtype=torch.int32, device="cuda"), rgba=torch.full((n + 1,), SENTINEL, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    host = {k: np.ascontiguousarray(v).copy() for k, v in a.items()}
    host.update(out=np.zeros((n, 8), F), halves_out=np.zeros((2 * n, 8), F), length_out=np.zeros(n, F), rgba=np.zeros((n, 4), np.uint8))
    prm, cam = hip.accumulate_params(frame_params(case)), case["cam"].c_struct()
    order = KEYS + ("out", "halves_out", "length_out", "rgba")

    def call(p):
        return L.rr_accumulate_records_device(small_scene._h, C.byref(cam), C.byref(prm), *(C.c_void_p(p[k]) if p[k] else None for k in order), None)

    good = {k: dev[k].data_ptr() for k in order}
    for key in order:                                               # a pageable pointer, refused by name
        rc = call(dict(good, **{key: host[key].ctypes.data}))
        assert rc == -1 and names[key] in L.rr_last_error(), (key, rc, L.rr_last_error())
    for key in order:                                               # misalignment
        rc = call(dict(good, **{key: good[key] + (4 if key in ("records", "halves", "history", "history_halves", "out", "halves_out") else 2)}))
        assert rc == -1 and b"aligned" in L.rr_last_error(), (key, rc, L.rr_last_error())
    assert call(dict(good, history=good["out"])) == -1 and b"out overlaps history" in L.rr_last_error()
    assert call(dict(good, halves_out=None)) == -1 and b"halves_out is required" in L.rr_last_error()
    assert call(dict(good, history_length=None)) == -1 and b"history and history_length" in L.rr_last_error()
    torch.cuda.synchronize()
    for k in ("out", "halves_out", "length_out", "rgba"):
        assert (dev[k].cpu().numpy().view(np.uint32) == SENTINEL).all(), k
    assert call(good) == 0                                          # and the same pointers, all good, are taken
    torch.cuda.synchronize()
    assert (dev["out"].cpu().numpy().view(np.uint32)[:n] != SENTINEL).any()


# ---- 3: end to end ------------------------------------------------------------------------------------------------------------------
def test_a_static_camera_over_six_frames(hip):
    """spheres_room, 50x38, 6 frames of 4 samples with 6 seeds: render_temporal (three calls on one stream, no host trip) equals
    render_pixel_parts -> the yardstick -> atrous_denoise frame by frame, bit for bit; before the filter the accumulated colour is the
    mean of the six frames up to the rounding of the incremental mean."""
    import torch
    from rustray_amd.renderer import Raytracing, TemporalState, _pack_records
    W, H = 50, 38
    fs = _scene("spheres_room")
    camera = camera_for(fs, W, H)
    rt = Raytracing(fs, camera, 0)
    try:
        rt.config = _cfg("plain", samples=4)
        state = TemporalState()
        hist = dict(records=None, halves=None, length=None)
        view = previous_view(camera)
        frames, frame_halves = [], []
        for k in range(6):
            got = rt.render_temporal(state, samples=4, seed=100 + k, rgba8=True)
            torch.cuda.synchronize()
            rt.config.seed = 100 + k
            base = rt.render_pixel_parts(n_parts=2)
            records, halves = _pack_records(base), _pack_records(base["parts"])
            frames.append(records[:, 0:3]); frame_halves.append(halves[:, :, 0:3])
            hist = accumulate_records(records, halves, hist["records"], hist["halves"], hist["length"], None, camera,
                                      AccumulateParams(prev_world_to_clip=view[0], prev_eye=view[1]))
            want = atrous_denoise(hist["records"], hist["halves"], None, W, H)
            np_ = lambda t: t.cpu().numpy().view(np.uint32)
            assert np.array_equal(np_(got["noisy"]), records.view(np.uint32)) and np.array_equal(np_(got["halves"]), halves.view(np.uint32)), k
            assert np.array_equal(np_(got["accumulated"]), hist["records"].view(np.uint32)), (k, int((np_(got["accumulated"]) != hist["records"].view(np.uint32)).sum()))
            assert np.array_equal(np_(got["accumulated_halves"]), hist["halves"].view(np.uint32)) and np.array_equal(np_(got["length"]), hist["length"].view(np.uint32)), k
            assert np.array_equal(np_(got["records"]), want["records"].view(np.uint32)), k
            assert np.array_equal(got["rgba"].cpu().numpy(), denoise.frame_bytes_linear(want["records"][:, 0:3])), k
        assert state.frames == 6
        # a static camera: every pixel with a surface under it kept all six frames; a miss (no history: a constant background) has its own
        fin = np.isfinite(hist["records"][:, 0:3]).all(-1)
        surface = fin & np.isfinite(hist["records"][:, 3]) & np.isfinite(hist["records"][:, 4:7]).all(-1)
        print(f"{int(surface.sum())} of {W * H} pixels show a surface; lengths {np.unique(hist['length'], return_counts=True)}")
        assert (hist["length"][surface] == 6).all() and (hist["length"][fin & ~surface] == 1).all()
        for got_c, layers in ((hist["records"][:, 0:3], np.stack(frames)), (hist["halves"][:, 0, 0:3], np.stack([h[:, 0] for h in frame_halves])),
                              (hist["halves"][:, 1, 0:3], np.stack([h[:, 1] for h in frame_halves]))):
            mean = layers[:, fin].astype(np.float64).mean(0)
            bound = 6 * 2.0 ** -22 * float(np.abs(layers[:, fin]).max())
            err = np.abs(got_c[fin].astype(np.float64) - mean)
            print(f"largest deviation from the mean of the six frames {float(err.max()):.3g}, bound {bound:.3g}")
            assert float(err.max()) <= bound
    finally:
        rt.device_scene.close()


def test_a_camera_yaw_between_two_frames(hip):
    """spheres_room, 50x38: the second frame is seen from a camera yawed by about 2 pixels.  The device equals the yardstick bit for
    bit, and every pixel that kept history (length 2) has a history tap of its own id."""
    import math
    from rustray_amd.renderer import _pack_records
    W, H = 50, 38
    fs = _scene("spheres_room")
    first_cam = camera_for(fs, W, H)
    st = first_cam.state()
    a = 2.0 * (2.0 * math.tan(first_cam.fov / 2.0) / H)          # about 2 pixels: a pixel is 2 tan(fov / 2) / H radians wide at the centre
    d = np.asarray(st["dir"], np.float64)
    st["dir"] = [d[0] * math.cos(a) - d[2] * math.sin(a), d[1], d[0] * math.sin(a) + d[2] * math.cos(a)]
    second_cam = type(first_cam).from_state(st)
    cfg = _cfg("plain", samples=4)
    with hip.DeviceScene(fs, 0) as ds:
        one = ds.render_pixel_parts(first_cam.c_struct(), cfg, None, n_parts=2)
        two = ds.render_pixel_parts(second_cam.c_struct(), cfg, None, n_parts=2)
        r1, h1, r2, h2 = _pack_records(one), _pack_records(one["parts"]), _pack_records(two), _pack_records(two["parts"])
        first = ds.accumulate_records(first_cam.c_struct(), r1, h1)
        m, eye = previous_view(first_cam)
        prm = AccumulateParams(prev_world_to_clip=m, prev_eye=eye)
        got = ds.accumulate_records(second_cam.c_struct(), r2, h2, first["records"], first["halves"], first["length"], None, prm)
    assert np.array_equal(first["records"].view(np.uint32), r1.view(np.uint32)) and np.array_equal(first["halves"].view(np.uint32), h1.view(np.uint32))
    want = accumulate_records(r2, h2, first["records"], first["halves"], first["length"], None, second_cam, prm)
    _check(got, want, "a yaw of two pixels")
    kept = want["length"] == 2
    taps = want["taps"]
    q = np.clip(taps["y"], 0, H - 1) * W + np.clip(taps["x"], 0, W - 1)
    own = (r1[:, 7].view(np.uint32)[q] == r2[:, 7].view(np.uint32)[:, None]) & taps["taken"]
    assert own[kept].any(1).all() and not taps["taken"][~kept].any()
    assert set(np.unique(want["length"])) <= {0.0, 1.0, 2.0}
    print(f"a yaw of about 2 pixels at {W}x{H}: {kept.mean():.3f} of the pixels kept their history")
    assert kept.any() and (~kept).any()


# ---- 4: the handle afterwards -------------------------------------------------------------------------------------------------------
def test_the_handle_renders_the_same_frame_before_and_after(hip):
    fs = _scene("spheres_room")
    cam = camera_for(fs, 50, 38).c_struct()
    cfg = _cfg("plain")
    with hip.DeviceScene(fs, 0) as fresh:
        want = fresh.render(cam, cfg, aux=True)
    with hip.DeviceScene(fs, 0) as ds:
        first = ds.render(cam, cfg, aux=True); stats = ds.stats()
        _check(_device_call(ds, 130, 70, True, True, False), _yardstick(130, 70, True, True, False), "on a handle with a frame")
        assert ds.stats() == stats                      # nothing of a frame's statistics is touched
        second = ds.render(cam, cfg, aux=True)
        for k in ("rgba", "normal", "depth", "object_id"):
            assert np.array_equal(first[k], second[k], equal_nan=True) and np.array_equal(first[k], want[k], equal_nan=True), k


def test_an_edit_and_destroy_wait_for_the_call_in_flight(hip):
    """The call is enqueued on a stream and the scene is edited, then destroyed, at once: both wait for it, and its outputs are whole."""
    import torch
    from tests.helpers import item_transforms
    W, H = 130, 70
    n = W * H
    case = temporal_frame(W, H)
    a = _inputs(case, True, True, False)
    want = _yardstick(W, H, True, True, False)
    fs = _scene("spheres_room")
    t, ti = item_transforms(fs, dx=0.4)
    src = {k: torch.from_numpy(np.ascontiguousarray(v).copy()).cuda() for k, v in a.items()}
    for edit in ("update_transforms", "destroy"):
        out = torch.full((n, 8), SENTINEL, dtype=torch.int32, device="cuda")
        out_h = torch.full((2 * n, 8), SENTINEL, dtype=torch.int32, device="cuda")
        length = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        ds = hip.DeviceScene(fs, 0)
        try:
            ds.accumulate_records_device(case["cam"].c_struct(), *(src[k].data_ptr() for k in KEYS), out.data_ptr(), out_h.data_ptr(), length.data_ptr(), None,
                                         frame_params(case), st.cuda_stream)
            if edit == "update_transforms":
                ds.update_transforms(t, ti)
        finally:
            ds.close()
        got = dict(records=out.cpu().numpy().view(np.uint32), halves=out_h.cpu().numpy().view(np.uint32).reshape(n, 2, 8), length=length.cpu().numpy().view(np.uint32))
        _check(got, want, f"behind {edit}")
        torch.cuda.synchronize()
