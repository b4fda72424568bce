"""rr_surface_pixels: the camera's G-buffer and albedo on the device.

THE CONTRACT is an identity: surface_pixels(cam) equals, byte for byte in all 128 bytes of every record, surface_rays(*pixel_rays(cam),
depth=1) on the same handle -- rr_surface_rays is held to the oracle by tests/test_gpu_surface_rays.py, pixel_rays to the host function by
tests/test_pixel_rays_host.py -- and albedo equals base_color[:, :3] there, 0 on misses.  Everything else is the surroundings of a frame
call: lists, refusals, each output alone, the device form, the frames and statistics around it, scene edits, and a camera so far away that
the top level has to be padded for it before the first launch.
Position: surface_at forms origin + direction * distance in the order of temporal.world_positions, so the bits are expected to be equal on
every hit; the test prints the count of hits where they are not and asserts it is 0."""
import ctypes as C

import numpy as np
import pytest
import torch

from rustray_amd import renderer
from rustray_amd.flat import SURFACE_HIT_DTYPE, make_config, rr_camera
from rustray_amd.pixel_rays import pixel_rays
from rustray_amd.temporal import world_positions
from tests.helpers import assert_frames_identical, camera_for, load_scene

pytestmark = pytest.mark.gpu

SCENES = ("rich", "spheres_room", "monkey")
SIZES = ((1, 1), (3, 2), (16, 8), (50, 38), (70, 41))
W, H = 50, 38
SENTINEL = 0x5a
_cache = {}


def _scene(name):
    if name == "rich":
        from tools.fuzz_parity import rich_scene   # 20 items (packet top level), every texture slot
        return rich_scene(9119)
    return load_scene(name)                        # spheres_room: 14 items, the per-ray walk; monkey: one untextured mesh


def _bytes(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(len(a), a.dtype.itemsize * int(np.prod(a.shape[1:])))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _case(hip, name):
    """One handle per scene for the whole module, and per frame size the whole-frame answer and the yardstick on the same handle."""
    if name not in _cache:
        fs = _scene(name)
        ds = hip.DeviceScene(fs, 0)
        c = dict(fs=fs, ds=ds, frames={})
        for w, h in SIZES:
            cam = camera_for(fs, w, h).c_struct()
            rec, alb = ds.surface_pixels(cam)
            o, d = pixel_rays(cam)
            want = ds.surface_rays(o, d, 1)
            for a in (rec, alb, want):
                a.setflags(write=False)
            c["frames"][(w, h)] = dict(cam=cam, rec=rec, alb=alb, want=want, o=o, d=d)
        _cache[name] = c
    return _cache[name]


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for c in _cache.values():
        c["ds"].close()
    _cache.clear()


# ---- the contract -------------------------------------------------------------------------------------------------------------------
def test_the_50x38_frames_hold_hits_and_misses(hip):
    """So that neither clause of the contract is vacuous: each scene's frame has hits, and the scenes whose frame has no miss are named
    (spheres_room is a closed room: every ray hits a wall)."""
    only_hits = []
    for name in SCENES:
        want = _case(hip, name)["frames"][(W, H)]["want"]
        n_hit = int((want["hit"] == 1).sum())
        print(f"surface_pixels {name} {W}x{H}: {n_hit} hits, {W * H - n_hit} misses")
        assert n_hit > 0, name
        if n_hit == W * H:
            only_hits.append(name)
    print(f"surface_pixels: scenes whose {W}x{H} frame has only hits: {only_hits}")
    assert len(set(SCENES) - set(only_hits)) >= 2     # the miss clause is checked on at least two scenes


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", SCENES)
def test_whole_frame_is_surface_rays_of_pixel_rays(hip, name, size):
    f = _case(hip, name)["frames"][size]
    rec, alb, want = f["rec"], f["alb"], f["want"]
    n = size[0] * size[1]
    assert rec.dtype == SURFACE_HIT_DTYPE and rec.shape == (n,) and alb.dtype == np.float32 and alb.shape == (n, 3)
    differ = np.flatnonzero((_bytes(rec) != _bytes(want)).any(1))
    assert len(differ) == 0, f"{name} {size}: {len(differ)} records differ, first {differ[:4]}"
    assert np.array_equal(_bits(alb), _bits(want["base_color"][:, :3]))
    miss = want["hit"] == 0
    assert not alb[miss].any() and not _bytes(rec[miss])[:, 8:].any() and (rec["item_index"][miss] == 0xffffffff).all()


@pytest.mark.parametrize("name", SCENES)
def test_position_is_world_positions_at_the_records_distance(hip, name):
    f = _case(hip, name)["frames"][(W, H)]
    rec = f["rec"]
    hit = rec["hit"] == 1
    records = np.zeros((W * H, 8), np.float32)
    records[:, 3] = rec["distance"]
    want = world_positions(records, f["cam"])
    differ = int((_bits(rec["position"][hit]) != _bits(want[hit])).any(1).sum())
    print(f"surface_pixels {name}: position differs from world_positions on {differ} of {int(hit.sum())} hits")
    assert differ == 0


# ---- lists --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_lists_answer_as_the_whole_frame(hip, name):
    c = _case(hip, name)
    f = c["frames"][(W, H)]
    rng = np.random.default_rng(7)
    for n in (1, 63, 64, 65, 257):
        x, y = rng.integers(0, W, n), rng.integers(0, H, n)
        if n > 2:
            x[n // 2], y[n // 2] = x[0], y[0]          # a duplicate, far from its twin
            x[-1], y[-1] = W - 1, H - 1
        rec, alb = c["ds"].surface_pixels(f["cam"], np.stack([x, y], 1))
        at = y * W + x
        assert np.array_equal(_bytes(rec), _bytes(f["rec"][at])), n
        assert np.array_equal(_bits(alb), _bits(f["alb"][at])), n
    assert len(c["ds"].surface_pixels(f["cam"], np.zeros((0, 2), np.int64), records=True, albedo=False)) == 0


def test_a_list_entry_outside_the_frame_is_refused(hip):
    c = _case(hip, "rich")
    ds, cam = c["ds"], c["frames"][(W, H)]["cam"]
    L = hip.lib()
    xy = np.array([3 | (4 << 16), 49 | (37 << 16), 50 | (0 << 16), 0 | (38 << 16)], np.uint32)
    out = np.full(4 * 128, SENTINEL, np.uint8)
    alb = np.full(4 * 12, SENTINEL, np.uint8)
    rc = L.rr_surface_pixels(ds._h, C.byref(cam), C.c_void_p(xy.ctypes.data), 4, C.c_void_p(out.ctypes.data), C.c_void_p(alb.ctypes.data))
    assert rc == -1 and b"pixel_xy[2] = (50, 0) lies outside the frame of 50x38" in L.rr_last_error()
    assert (out == SENTINEL).all() and (alb == SENTINEL).all()
    # the device form learns it from the device: the same refusal, nothing written, no kernel reads past the frame, and no fault
    t_xy = torch.from_numpy(xy.view(np.int32)).cuda()
    t_out = torch.full((4 * 128,), SENTINEL, dtype=torch.uint8, device="cuda")
    t_alb = torch.full((4 * 12,), SENTINEL, dtype=torch.uint8, device="cuda")
    rc = L.rr_surface_pixels_device(ds._h, C.byref(cam), C.c_void_p(t_xy.data_ptr()), 4, C.c_void_p(t_out.data_ptr()), C.c_void_p(t_alb.data_ptr()), None)
    assert rc == -1 and b"pixel_xy[2] = (50, 0) lies outside the frame of 50x38" in L.rr_last_error()
    torch.cuda.synchronize()
    assert (t_out.cpu().numpy() == SENTINEL).all() and (t_alb.cpu().numpy() == SENTINEL).all()
    rec = ds.surface_pixels(cam, xy[:2], albedo=False)    # and the handle answers afterwards
    assert np.array_equal(_bytes(rec), _bytes(c["frames"][(W, H)]["rec"][[4 * W + 3, 37 * W + 49]]))


# ---- each output alone --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ((W, H), (3, 2)))
def test_each_output_alone_and_the_bytes_behind_it(hip, size):
    c = _case(hip, "rich")
    f = c["frames"][size]
    n = size[0] * size[1]
    L, h, cam = hip.lib(), c["ds"]._h, f["cam"]
    for records, albedo in ((True, False), (False, True), (True, True)):
        out = np.full(n * 128 + 64, SENTINEL, np.uint8)
        alb = np.full(n * 12 + 64, SENTINEL, np.uint8)
        assert L.rr_surface_pixels(h, C.byref(cam), None, n, C.c_void_p(out.ctypes.data) if records else None, C.c_void_p(alb.ctypes.data) if albedo else None) == 0
        assert np.array_equal(out[:n * 128].reshape(n, 128), _bytes(f["rec"])) if records else (out == SENTINEL).all()
        assert np.array_equal(alb[:n * 12].view(np.uint32).reshape(n, 3), _bits(f["alb"])) if albedo else (alb == SENTINEL).all()
        assert (out[n * 128:] == SENTINEL).all() and (alb[n * 12:] == SENTINEL).all()
        # the device form, whole frame
        t_out = torch.full((n * 128 + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        t_alb = torch.full((n * 12 + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        c["ds"].surface_pixels_device(cam, None, n, t_out.data_ptr() if records else None, t_alb.data_ptr() if albedo else None)
        torch.cuda.synchronize()
        g_out, g_alb = t_out.cpu().numpy(), t_alb.cpu().numpy()
        assert np.array_equal(g_out[:n * 128].reshape(n, 128), _bytes(f["rec"])) if records else (g_out == SENTINEL).all()
        assert np.array_equal(g_alb[:n * 12].view(np.uint32).reshape(n, 3), _bits(f["alb"])) if albedo else (g_alb == SENTINEL).all()
        assert (g_out[n * 128:] == SENTINEL).all() and (g_alb[n * 12:] == SENTINEL).all()
    assert c["ds"].surface_pixels(cam, albedo=False).dtype == SURFACE_HIT_DTYPE and c["ds"].surface_pixels(cam, records=False).shape == (n, 3)


# ---- the device form ----------------------------------------------------------------------------------------------------------------
def test_device_form_on_a_stream_behind_a_producer(hip):
    c = _case(hip, "rich")
    f = c["frames"][(W, H)]
    ds, cam, n = c["ds"], f["cam"], W * H
    rng = np.random.default_rng(11)
    xy = (rng.integers(0, W, 257) | (rng.integers(0, H, 257) << 16)).astype(np.uint32)
    at = (xy >> 16) * W + (xy & 0xffff)
    st = torch.cuda.Stream()
    src = torch.from_numpy(xy.view(np.int32)).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        whole = renderer.surface_pixels_torch(ds, cam)
        listed = renderer.surface_pixels_torch(ds, cam, src + 0)      # the list is produced on the stream the query runs on
        only = renderer.surface_pixels_torch(ds, cam, records=False)
    st.synchronize()
    rec = whole["records"]
    assert rec.shape == (n, 32) and rec.dtype == torch.float32 and rec.is_cuda and whole["albedo"].shape == (n, 3)
    assert np.array_equal(rec.cpu().numpy().view(np.uint8).reshape(n, 128), _bytes(f["rec"]))
    assert np.array_equal(_bits(whole["albedo"].cpu().numpy()), _bits(f["alb"]))
    assert np.array_equal(listed["records"].cpu().numpy().view(np.uint8).reshape(257, 128), _bytes(f["rec"][at]))
    assert np.array_equal(_bits(listed["albedo"].cpu().numpy()), _bits(f["alb"][at]))
    assert set(only) == {"albedo"} and np.array_equal(_bits(only["albedo"].cpu().numpy()), _bits(f["alb"]))
    for name in SURFACE_HIT_DTYPE.names:   # named column views of the one tensor: no copy
        assert whole[name].untyped_storage().data_ptr() == rec.untyped_storage().data_ptr(), name
    assert np.array_equal(_bits(whole["base_color"].cpu().numpy()[:, :3]), _bits(f["alb"]))
    with pytest.raises(ValueError):
        renderer.surface_pixels_torch(ds, cam, src.cpu())
    with pytest.raises(ValueError):
        renderer.surface_pixels_torch(ds, cam, records=False, albedo=False)


def test_device_form_refusals_launch_nothing(hip):
    c = _case(hip, "rich")
    f = c["frames"][(W, H)]
    L, h, cam, n = hip.lib(), c["ds"]._h, f["cam"], W * H
    buf = torch.full((n * 128 + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    alb = torch.full((n * 12 + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    xy = torch.zeros((n,), dtype=torch.int32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    dev = lambda p_xy, p_out, p_alb: L.rr_surface_pixels_device(h, C.byref(cam), p_xy, n, p_out, p_alb, None)
    P = lambda v: C.c_void_p(v)
    for off in (4, 8, 12):
        assert dev(None, P(buf.data_ptr() + off), P(alb.data_ptr())) == -1
        assert b"rr_surface_pixels_device" in L.rr_last_error() and b"out_dev is not 16-byte aligned" in L.rr_last_error()
    assert dev(None, P(buf.data_ptr()), P(alb.data_ptr() + 2)) == -1 and b"albedo_out_dev is not 4-byte aligned" in L.rr_last_error()
    assert dev(P(xy.data_ptr() + 1), P(buf.data_ptr()), None) == -1 and b"pixel_xy_dev is not 4-byte aligned" in L.rr_last_error()
    # overlap: the outputs with each other, and each with the list
    assert dev(None, P(buf.data_ptr()), P(buf.data_ptr() + n * 128 - 16)) == -1 and b"albedo_out_dev overlaps out_dev" in L.rr_last_error()
    assert dev(P(buf.data_ptr() + 64), P(buf.data_ptr()), None) == -1 and b"out_dev overlaps pixel_xy_dev" in L.rr_last_error()
    assert dev(P(alb.data_ptr() + 8), None, P(alb.data_ptr())) == -1 and b"albedo_out_dev overlaps pixel_xy_dev" in L.rr_last_error()
    # pageable host memory, by argument name
    host = np.zeros(n * 128 + 16, np.uint8)
    ph = host.ctypes.data + (-host.ctypes.data) % 16
    assert dev(None, P(ph), P(alb.data_ptr())) == -1 and b"out_dev" in L.rr_last_error() and b"cannot address" in L.rr_last_error()
    assert dev(None, P(buf.data_ptr()), P(ph)) == -1 and b"albedo_out_dev" in L.rr_last_error()
    assert dev(P(ph), P(buf.data_ptr()), None) == -1 and b"pixel_xy_dev" in L.rr_last_error()
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == SENTINEL).all() and (alb.cpu().numpy() == SENTINEL).all() and not host.any()
    # and the handle answers afterwards
    assert dev(None, P(buf.data_ptr()), P(alb.data_ptr())) == 0
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy()[:n * 128].reshape(n, 128), _bytes(f["rec"]))


# ---- surroundings -------------------------------------------------------------------------------------------------------------------
def test_frames_and_statistics_around_the_call_are_unchanged(hip):
    c = _case(hip, "rich")
    f = c["frames"][(W, H)]
    ds, cam = c["ds"], f["cam"]
    cfg = make_config(samples=3, monte_carlo=True, seed=3, max_recursion=4)
    before = ds.render(cam, cfg, aux=True)
    stats = ds.stats()
    rec, alb = ds.surface_pixels(cam)
    listed = ds.surface_pixels(cam, np.array([[1, 2], [40, 30]]), albedo=False)
    assert ds.stats() == stats
    after = ds.render(cam, cfg, aux=True)
    assert np.array_equal(_bytes(rec), _bytes(f["rec"])) and np.array_equal(_bytes(listed), _bytes(f["rec"][[2 * W + 1, 30 * W + 40]]))
    assert_frames_identical(before, after, "rr_render around rr_surface_pixels")


def test_after_scene_edits_the_call_answers_as_a_new_handle(hip):
    def edit(drop_item):
        out = _scene("rich")
        for k, m in enumerate(out.materials):
            m.ambient_color, m.base_color, m.specular_color = tuple(m.base_color), tuple(m.specular_color), tuple(m.ambient_color)
            m.roughness, m.reflectivity = 0.125 + 0.01 * k, 0.25
            m.texture = list(m.texture[1:]) + [m.texture[0]]
        if drop_item:
            del out.items[3]
        return out
    edited, fewer = edit(False), edit(True)
    cam = camera_for(edited, W, H).c_struct()
    with hip.DeviceScene(edited, 0) as ds:
        want_materials = ds.surface_pixels(cam)
    with hip.DeviceScene(fewer, 0) as ds:
        want_items = ds.surface_pixels(cam)
    first = _case(hip, "rich")["frames"][(W, H)]
    with hip.DeviceScene(_scene("rich"), 0) as ds:
        got = ds.surface_pixels(cam)
        assert np.array_equal(_bytes(got[0]), _bytes(first["rec"])) and np.array_equal(_bits(got[1]), _bits(first["alb"]))
        ds.update_materials(edited.materials)
        got = ds.surface_pixels(cam)
        assert np.array_equal(_bytes(got[0]), _bytes(want_materials[0])) and np.array_equal(_bits(got[1]), _bits(want_materials[1]))
        assert not np.array_equal(_bits(got[1]), _bits(first["alb"]))
        ds.set_items(fewer.items, fewer.materials)
        got = ds.surface_pixels(cam)
        assert np.array_equal(_bytes(got[0]), _bytes(want_items[0])) and np.array_equal(_bits(got[1]), _bits(want_items[1]))
        assert not np.array_equal(_bytes(got[0]), _bytes(want_materials[0]))


@pytest.mark.parametrize("name", ("rich", "spheres_room"))
def test_a_far_camera_answers_as_surface_rays(hip, name):
    """The eye 10^4 scene sizes behind where it stood (a scene size: the median distance of the near frame's hits), with the lens that much
    longer, so that the scene fills the frame as before.  The origins lie far outside anything the handle has been padded for, and the
    call's first launch follows the host's own bound: the answer is surface_rays' on a fresh handle, which reads the reach back from the
    device, and it holds hits."""
    fs = _scene(name)
    near = _case(hip, name)["frames"][(W, H)]
    size = float(np.median(near["rec"]["distance"][near["rec"]["hit"] == 1]))
    far = rr_camera.from_buffer_copy(near["cam"])
    back = np.array(far.view_inverse[8:11], np.float64)
    back /= np.linalg.norm(back)
    for k in range(3):
        far.view_inverse[12 + k] = float(np.float32(far.view_inverse[12 + k] + back[k] * 1e4 * size))
    zoom = 1e4 + 1.0
    for k in range(4):
        far.projection_inverse[k] = float(np.float32(far.projection_inverse[k] / zoom))
        far.projection_inverse[4 + k] = float(np.float32(far.projection_inverse[4 + k] / zoom))
    o, d = pixel_rays(far)
    assert float(np.abs(o).max()) > 1e3 * size
    with hip.DeviceScene(fs, 0) as ds:
        rec, alb = ds.surface_pixels(far)              # the first call of a fresh handle: only the host bound can have padded the top level
        same_handle = ds.surface_rays(o, d, 1)
        again = ds.surface_pixels(far, albedo=False)
    with hip.DeviceScene(fs, 0) as ds:
        want = ds.surface_rays(o, d, 1)
    n_hit = int((want["hit"] == 1).sum())
    print(f"surface_pixels {name} far camera: {n_hit} hits of {W * H}")
    assert n_hit > 0
    assert np.array_equal(_bytes(rec), _bytes(want)) and np.array_equal(_bytes(same_handle), _bytes(want)) and np.array_equal(_bytes(again), _bytes(want))
    assert np.array_equal(_bits(alb), _bits(want["base_color"][:, :3]))
