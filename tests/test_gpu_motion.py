"""rr_motion_records on the device against the numpy yardstick temporal.motion_records, every output word equal.

1: the hand-made frame and items of tests/motion_cases.py at 37x19 and 130x70 (several workgroups both ways; waves of one id and waves
whose ids alternate lane by lane; ids 0 and 0xffffffff; misses, NaN, inf and 3e38 depths) with 0, 1, 3 and 70 moved items, with and
without world_out, sentinels behind both outputs, the records unchanged, behind its producer on a non-null stream; 2: the host form, the
transforms the handle holds NOW, refusals that launch nothing; 3: end to end on spheres_room -- a sphere moved by about two pixels between
two frames of a static camera; 4: the handle afterwards, an edit and a destroy behind a call in flight."""
import ctypes as C

import numpy as np
import pytest

from rustray_amd.denoise import atrous_denoise
from rustray_amd.temporal import AccumulateParams, accumulate_records, motion_records, previous_view
from tests.denoise_cases import F, differing_words
from tests.helpers import camera_for, item_transforms, with_transforms
from tests.motion_cases import N_ITEMS, N_MOVED, motion_frame, motion_items, motion_scene, moved_list
from tests.test_gpu_pixel_parts import SENTINEL, _cfg
from tests.test_gpu_shade_rays import _scene

pytestmark = pytest.mark.gpu

SIZES = ((37, 19), (130, 70))
_want = {}


def _yardstick(W, H, n_moved):
    """The yardstick's answer for motion_frame(W, H) and the first n_moved items of the list, computed once and left unchanged."""
    if (W, H, n_moved) not in _want:
        it, case = motion_items(), motion_frame(W, H)
        idx, prev = moved_list(n_moved)
        motion, world = motion_records(case["records"], case["cam"], it["ids"][idx], prev, it["trans_inv"][idx])
        motion.setflags(write=False); world.setflags(write=False)
        _want[(W, H, n_moved)] = (motion, world)
    return _want[(W, H, n_moved)]


@pytest.fixture(scope="module")
def items_scene(hip):
    with hip.DeviceScene(motion_scene(), 0) as ds:
        yield ds


def _check(got, want, what, world=True):
    differ, nans = differing_words(got["motion"], want[0])
    assert differ == 0 and nans == 0, f"{what}: {differ} of {want[0].size} words of motion differ ({nans} NaNs)"
    if world:
        differ, nans = differing_words(got["world"], want[1])
        if nans:
            print(f"{what}: {nans} words of world are NaNs of other bits on both sides")
        assert differ == 0, f"{what}: {differ} of {want[1].size} words of world differ"


def _device_call(ds, W, H, n_moved, world=True, stream=None, produce=False):
    """One rr_motion_records_device call on motion_frame(W, H) with sentinels behind both outputs -> dict(motion, world) as float32.
    produce: the records are made by a copy kernel on `stream` and the call follows it without a synchronisation."""
    import torch
    n = W * H
    case = motion_frame(W, H)
    idx, prev = moved_list(n_moved)
    ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.device(0)
    with ctx:
        rec = torch.from_numpy(case["records"].copy()).cuda()
        motion = torch.full((n + 2, 3), SENTINEL, dtype=torch.int32, device="cuda")
        wout = torch.full((n + 2, 3), SENTINEL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        if produce:
            rec = rec.clone()          # (a copy kernel on `stream`; the call is enqueued behind it)
        ds.motion_records_device(case["cam"].c_struct(), idx, prev, rec.data_ptr(), motion.data_ptr(), wout.data_ptr() if world else None,
                                 stream.cuda_stream if stream is not None else None)
    torch.cuda.synchronize()
    m, w = motion.cpu().numpy().view(np.uint32), wout.cpu().numpy().view(np.uint32)
    assert (m[n:] == SENTINEL).all() and (w[n:] == SENTINEL).all(), "words behind an output were written"
    if not world:
        assert (w == SENTINEL).all()
    assert np.array_equal(rec.cpu().numpy().view(np.uint32), case["records"].view(np.uint32)), "the records were written"
    return dict(motion=m[:n].view(F), world=w[:n].view(F))


# ---- 1: the hand-made frame against the yardstick -----------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("n_moved", N_MOVED)
@pytest.mark.parametrize("world", (True, False))
def test_every_word_equals_the_yardstick(items_scene, W, H, n_moved, world):
    want = _yardstick(W, H, n_moved)
    assert (want[0] != 0).any() == (n_moved > 0)
    _check(_device_call(items_scene, W, H, n_moved, world=world), want, f"{W}x{H} n_moved={n_moved} world={world}", world=world)


def test_after_its_producer_on_a_non_null_stream(items_scene):
    import torch
    st = torch.cuda.Stream()
    _check(_device_call(items_scene, 130, 70, 70, stream=st, produce=True), _yardstick(130, 70, 70), "behind its producer")
    _check(_device_call(items_scene, 130, 70, 3, stream=st, produce=True), _yardstick(130, 70, 3), "behind its producer, a shorter list")
    _check(_device_call(items_scene, 37, 19, 0, world=False, stream=st, produce=True), _yardstick(37, 19, 0), "behind its producer, nothing moved", world=False)


def test_calls_back_to_back_keep_their_own_tables(items_scene):
    """Nine calls with different lists on one stream behind a slow producer, not waited for in between: more calls than the handle has
    pinned copies of the table (four, used in turn), so a copy is written again while the calls that read it are still queued -- a call's
    table must reach that call alone, and a pinned copy must not be overwritten before its reader has run."""
    import torch
    W, H = 130, 70
    n = W * H
    case = motion_frame(W, H)
    lists = (70, 1, 3, 70, 3, 1, 70, 1, 3)
    outs = [torch.zeros((n, 3), device="cuda") for _ in lists]
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        src = torch.from_numpy(case["records"].copy()).cuda()
        a = torch.rand((4096, 4096), device="cuda")
        torch.cuda.synchronize()
        for _ in range(40):                      # the slow producer: some tens of milliseconds of work queued ahead of the records
            a = (a @ a).clamp_(0, 1)
        rec = src.clone()
        for out, k in zip(outs, lists):
            idx, prev = moved_list(k)
            items_scene.motion_records_device(case["cam"].c_struct(), idx, prev, rec.data_ptr(), out.data_ptr(), None, st.cuda_stream)
    torch.cuda.synchronize()
    for i, (out, k) in enumerate(zip(outs, lists)):
        _check(dict(motion=out.cpu().numpy()), _yardstick(W, H, k), f"call {i} with n_moved={k}", world=False)


# ---- 2: the host form, the handle's current transforms, refusals --------------------------------------------------------------------
def test_device_form_equals_host_form(items_scene):
    W, H = 130, 70
    case = motion_frame(W, H)
    for n_moved in (70, 0):
        idx, prev = moved_list(n_moved)
        motion, world = items_scene.motion_records(case["cam"].c_struct(), idx, prev, case["records"], world=True)
        dev = _device_call(items_scene, W, H, n_moved)
        assert np.array_equal(motion.view(np.uint32), dev["motion"].view(np.uint32)) and np.array_equal(world.view(np.uint32), dev["world"].view(np.uint32))
        _check(dict(motion=motion, world=world), _yardstick(W, H, n_moved), f"host form, n_moved={n_moved}")
        only, none = items_scene.motion_records(case["cam"].c_struct(), idx, prev, case["records"])
        assert none is None and np.array_equal(only.view(np.uint32), motion.view(np.uint32))
    idx, prev = moved_list(3)                    # a refused list comes back from the host form as well, before anything is staged
    with pytest.raises(Exception, match="entries 0 and 2"):
        items_scene.motion_records(case["cam"].c_struct(), [idx[0], idx[1], idx[0]], prev, case["records"])


def test_the_inverse_is_the_one_the_handle_holds_now(hip):
    """After rr_scene_update_transforms the call uses the new trans_inv: the one the current frame is traced with."""
    W, H = 37, 19
    it, case = motion_items(), motion_frame(W, H)
    idx, prev = moved_list(70)
    new_t, new_ti = it["trans"].copy(), it["trans_inv"].copy()
    shift = np.eye(4, dtype=np.float64)
    shift[:3, 3] = (0.25, -0.5, 0.125)
    for i in idx[:40]:
        new_t[i] = (shift @ it["trans"][i].astype(np.float64)).astype(F)
        new_ti[i] = np.linalg.inv(shift @ it["trans"][i].astype(np.float64)).astype(F)
    want = motion_records(case["records"], case["cam"], it["ids"][idx], prev, new_ti[idx])
    assert (want[0] != _yardstick(W, H, 70)[0]).any()
    with hip.DeviceScene(motion_scene(), 0) as ds:
        before = ds.motion_records(case["cam"].c_struct(), idx, prev, case["records"], world=True)
        _check(dict(motion=before[0], world=before[1]), _yardstick(W, H, 70), "before the update")
        ds.update_transforms(new_t, new_ti)
        after = ds.motion_records(case["cam"].c_struct(), idx, prev, case["records"], world=True)
        _check(dict(motion=after[0], world=after[1]), want, "after the update")


def test_refusals_launch_nothing(items_scene, hip):
    import torch
    L = hip.lib()
    W, H = 37, 19
    n = W * H
    it, case = motion_items(), motion_frame(W, H)
    cam = case["cam"].c_struct()
    rec = torch.from_numpy(case["records"].copy()).cuda()
    motion = torch.full((n + 1, 3), SENTINEL, dtype=torch.int32, device="cuda")
    wout = torch.full((n + 1, 3), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    host = dict(records=case["records"].copy(), motion=np.zeros((n, 3), F), world=np.zeros((n, 3), F))
    good = dict(records=rec.data_ptr(), motion=motion.data_ptr(), world=wout.data_ptr())
    names = dict(records=b"records_dev", motion=b"motion_out_dev", world=b"world_out_dev")
    idx, prev = moved_list(3)
    cm = lambda p: np.ascontiguousarray(np.transpose(p, (0, 2, 1)))

    def call(p, index=idx, trans=cm(prev), k=None):
        k = len(index) if k is None else k
        return L.rr_motion_records_device(items_scene._h, C.byref(cam), index.ctypes.data_as(C.c_void_p) if index is not None else None,
                                          trans.ctypes.data_as(C.c_void_p) if trans is not None else None, C.c_uint32(k),
                                          *(C.c_void_p(p[key]) if p[key] else None for key in ("records", "motion", "world")), None)

    for key in names:                                               # a pageable pointer, refused by name
        rc = call(dict(good, **{key: host[key].ctypes.data}))
        assert rc == -1 and names[key] in L.rr_last_error(), (key, rc, L.rr_last_error())
    for key in names:                                               # misalignment
        rc = call(dict(good, **{key: good[key] + (4 if key == "records" else 2)}))
        assert rc == -1 and b"aligned" in L.rr_last_error(), (key, rc, L.rr_last_error())
    assert call(dict(good, world=good["motion"] + 12)) == -1 and b"world_out overlaps motion_out" in L.rr_last_error()
    assert call(dict(good, motion=good["records"] + 32)) == -1 and b"motion_out overlaps records" in L.rr_last_error()
    assert call(dict(good, motion=None)) == -1 and b"motion_out is NULL" in L.rr_last_error()
    assert call(good, index=None, k=3) == -1 and b"item_index is NULL" in L.rr_last_error()
    assert call(good, trans=None, k=3) == -1 and b"prev_trans is NULL" in L.rr_last_error()
    # the table builder's refusals, through the call
    many = np.arange(N_ITEMS + 1, dtype=np.uint32) % N_ITEMS
    assert call(good, index=many, trans=cm(np.tile(prev[:1], (N_ITEMS + 1, 1, 1)))) == -1 and b"n_moved 81" in L.rr_last_error()
    assert call(good, index=np.array([idx[0], N_ITEMS, idx[2]], np.uint32)) == -1 and b"item_index[1] = 80" in L.rr_last_error()
    assert call(good, index=np.array([idx[0], idx[1], idx[0]], np.uint32)) == -1 and b"entries 0 and 2" in L.rr_last_error()
    bad = cm(prev).copy()
    bad[2, 3, 1] = np.inf
    assert call(good, trans=bad) == -1 and b"prev_trans of entry 2 is not finite" in L.rr_last_error()
    torch.cuda.synchronize()
    assert (motion.cpu().numpy().view(np.uint32) == SENTINEL).all() and (wout.cpu().numpy().view(np.uint32) == SENTINEL).all()
    assert call(good) == 0                                          # and the same pointers, all good, are taken
    torch.cuda.synchronize()
    _check(dict(motion=motion.cpu().numpy()[:n].view(F), world=wout.cpu().numpy()[:n].view(F)), _yardstick(W, H, 3), "after the refusals")


def test_torch_glue(items_scene):
    import torch
    from rustray_amd.renderer import TemporalState, motion_torch, render_temporal_torch
    W, H = 37, 19
    case = motion_frame(W, H)
    idx, prev = moved_list(3)
    rec = torch.from_numpy(case["records"].copy()).cuda()
    got = motion_torch(items_scene, case["cam"].c_struct(), rec, idx, prev, world=True)
    torch.cuda.synchronize()
    _check(dict(motion=got["motion"].cpu().numpy(), world=got["world"].cpu().numpy()), _yardstick(W, H, 3), "motion_torch")
    assert motion_torch(items_scene, case["cam"].c_struct(), rec, idx, prev)["world"] is None
    with pytest.raises(ValueError):
        motion_torch(items_scene, case["cam"].c_struct(), rec[:-1], idx, prev)
    with pytest.raises(ValueError):
        render_temporal_torch(items_scene, case["cam"].c_struct(), _cfg("plain", samples=4), TemporalState(), motion=got["motion"], moved=(idx, prev))


# ---- 3: end to end ------------------------------------------------------------------------------------------------------------------
def test_a_sphere_moved_by_two_pixels_between_two_frames(hip):
    """spheres_room, 50x38, 4 samples in two halves, a static camera, two frames; between them one sphere is translated by about two
    pixels through apply_scene.  render_temporal(track_items=True) -- four calls on one stream -- equals render_pixel_parts ->
    motion_records -> accumulate_records -> atrous_denoise in numpy, bit for bit; and among the moved sphere's pixels more keep their
    history (length 2) with the motion than without (as measured: 0.919 against 0.441 of the 111 pixels of the sphere of id 42)."""
    import math
    import torch
    from rustray_amd.flat import RR_ITEM_SPHERE
    from rustray_amd.renderer import Raytracing, TemporalState, _pack_records
    W, H = 50, 38
    fs = _scene("spheres_room")
    camera = camera_for(fs, W, H)
    rt = Raytracing(fs, camera, 0)
    try:
        rt.config = _cfg("plain", samples=4)
        state = TemporalState()
        view = previous_view(camera)
        prm = AccumulateParams(prev_world_to_clip=view[0], prev_eye=view[1])
        np_ = lambda t: t.cpu().numpy().view(np.uint32)

        def frame(seed):
            got = rt.render_temporal(state, samples=4, seed=seed, track_items=True)
            torch.cuda.synchronize()
            rt.config.seed = seed
            base = rt.render_pixel_parts(n_parts=2)
            return got, _pack_records(base), _pack_records(base["parts"])

        got, r1, h1 = frame(100)
        assert got["motion"] is None
        first = accumulate_records(r1, h1, None, None, None, None, camera, prm)
        assert np.array_equal(np_(got["accumulated"]), first["records"].view(np.uint32))
        # the sphere that covers the most pixels, and at least 50
        ids1 = r1[:, 7].view(np.uint32)
        surface = np.isfinite(r1[:, 3]) & np.isfinite(r1[:, 4:7]).all(-1)
        cover = {i: int(((ids1 == np.uint32(it.id)) & surface).sum()) for i, it in enumerate(fs.items) if it.kind == RR_ITEM_SPHERE}
        item = max(cover, key=cover.get)
        assert cover[item] >= 50, cover
        ident = np.uint32(fs.items[item].id)
        # about two pixels to the camera's right at the sphere's depth: a pixel is 2 tan(fov / 2) / H wide one unit ahead of the eye
        d, up = np.asarray(camera.dir, np.float64), np.asarray(camera.up, np.float64)
        right = np.cross(d, up) / np.linalg.norm(np.cross(d, up))
        depth = float(np.median(r1[(ids1 == ident) & surface, 3])) + 1.0
        step = 2.0 * depth * 2.0 * math.tan(camera.fov / 2.0) / H
        t, ti = item_transforms(fs)
        move, back = np.eye(4), np.eye(4)
        move[:3, 3], back[:3, 3] = right * step, -right * step
        old = t[item].copy()
        t[item], ti[item] = (move @ t[item].astype(np.float64)).astype(F), (ti[item].astype(np.float64) @ back).astype(F)
        plan = rt.apply_scene(with_transforms(_scene("spheres_room"), t, ti))      # (a fresh copy: fs holds its ABI view by now)
        assert plan == ["update_transforms"], plan

        got, r2, h2 = frame(101)
        motion, _ = motion_records(r2, camera, [ident], old[None], ti[item][None])
        with_motion = accumulate_records(r2, h2, first["records"], first["halves"], first["length"], motion, camera, prm)
        without = accumulate_records(r2, h2, first["records"], first["halves"], first["length"], None, camera, prm)
        want = atrous_denoise(with_motion["records"], with_motion["halves"], None, W, H)
        assert np.array_equal(np_(got["noisy"]), r2.view(np.uint32)) and np.array_equal(np_(got["halves"]), h2.view(np.uint32))
        assert np.array_equal(np_(got["motion"]), motion.view(np.uint32)), int((np_(got["motion"]) != motion.view(np.uint32)).sum())
        assert np.array_equal(np_(got["accumulated"]), with_motion["records"].view(np.uint32))
        assert np.array_equal(np_(got["accumulated_halves"]), with_motion["halves"].view(np.uint32)) and np.array_equal(np_(got["length"]), with_motion["length"].view(np.uint32))
        assert np.array_equal(np_(got["records"]), want["records"].view(np.uint32))
        assert state.frames == 2
        on_sphere = (r2[:, 7].view(np.uint32) == ident) & np.isfinite(r2[:, 3]) & np.isfinite(r2[:, 4:7]).all(-1)
        share_with, share_without = float((with_motion["length"][on_sphere] == 2).mean()), float((without["length"][on_sphere] == 2).mean())
        shift = np.linalg.norm(motion[on_sphere], axis=1)
        print(f"item {item} (id {int(ident)}): {int(on_sphere.sum())} pixels, moved by {step:.4f} (|motion| {shift.min():.4f} .. {shift.max():.4f}); "
              f"length == 2 on {share_with:.3f} of them with the motion, {share_without:.3f} without")
        assert on_sphere.sum() >= 50 and np.allclose(shift, step, rtol=1e-3)
        assert not motion[~on_sphere].any()
        assert share_with > share_without
    finally:
        rt.device_scene.close()


# ---- 4: the handle afterwards -------------------------------------------------------------------------------------------------------
def test_the_handle_renders_the_same_frame_before_and_after(hip):
    fs = _scene("spheres_room")
    cam = camera_for(fs, 50, 38).c_struct()
    cfg = _cfg("plain")
    t, _ = item_transforms(fs, dx=0.3)
    with hip.DeviceScene(fs, 0) as fresh:
        want = fresh.render(cam, cfg, aux=True)
    with hip.DeviceScene(fs, 0) as ds:
        first = ds.render(cam, cfg, aux=True); stats = ds.stats()
        from rustray_amd.renderer import _pack_records
        records = _pack_records(ds.render_pixels(cam, cfg, None))
        stats = ds.stats()
        index = np.arange(len(fs.items), dtype=np.uint32)
        motion, world = ds.motion_records(cam, index, t, records, world=True)
        ti_now = np.stack([np.asarray(it.trans_inv, F) for it in fs.items])
        want_motion = motion_records(records, cam, [it.id for it in fs.items], t, ti_now)
        _check(dict(motion=motion, world=world), want_motion, "on a handle with a frame")
        assert (motion != 0).any()
        assert ds.stats() == stats                      # nothing of a frame's statistics is touched
        second = ds.render(cam, cfg, aux=True)
        for k in ("rgba", "normal", "depth", "object_id"):
            assert np.array_equal(first[k], second[k], equal_nan=True) and np.array_equal(first[k], want[k], equal_nan=True), k


def test_an_edit_and_destroy_wait_for_the_call_in_flight(hip):
    """The call is enqueued on a stream and the scene is edited, then destroyed, at once: both wait for it, and its outputs are whole
    (and those of the transforms the handle held when the call was made)."""
    import torch
    W, H = 130, 70
    n = W * H
    it, case = motion_items(), motion_frame(W, H)
    idx, prev = moved_list(70)
    want = _yardstick(W, H, 70)
    fs = motion_scene()
    t, ti = item_transforms(fs, dx=0.4)
    rec = torch.from_numpy(case["records"].copy()).cuda()
    for edit in ("update_transforms", "destroy"):
        motion = torch.full((n, 3), SENTINEL, dtype=torch.int32, device="cuda")
        wout = torch.full((n, 3), SENTINEL, dtype=torch.int32, device="cuda")
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        ds = hip.DeviceScene(fs, 0)
        try:
            ds.motion_records_device(case["cam"].c_struct(), idx, prev, rec.data_ptr(), motion.data_ptr(), wout.data_ptr(), st.cuda_stream)
            if edit == "update_transforms":
                ds.update_transforms(t, ti)
        finally:
            ds.close()
        _check(dict(motion=motion.cpu().numpy().view(F), world=wout.cpu().numpy().view(F)), want, f"behind {edit}")
        torch.cuda.synchronize()
