"""The promises of the progressive entry points (include/rustray_hip.h), through ctypes with caller buffers that start out as
garbage: pixels not rendered yet are zero -- also when the frame is cancelled before its first pass --, a stopped tile frame holds
exactly its finished tiles, and on_pass may ask its own scene for the statistics so far, while any other call on that scene is
refused instead of deadlocking on the scene's lock."""
import ctypes as C

import numpy as np
import pytest

from rustray_amd import capi
from rustray_amd.flat import make_config, rr_frame, rr_frame_stats
from rustray_amd.renderer import region_pixels
from tests.helpers import assert_frames_identical, camera_for, load_scene

pytestmark = pytest.mark.gpu

W, H = 100, 40   # 4 x 5 tiles of 32x8, the right column clipped
NAN_BITS = 0x7FC0A5A5   # a quiet NaN with a payload: no kernel writes this


def _sentinel_frame():
    out = dict(rgba=np.full((H, W, 4), 0xA5, np.uint8),
               normal=np.full((H, W, 3), NAN_BITS, np.uint32).view(np.float32),
               depth=np.full((H, W), NAN_BITS, np.uint32).view(np.float32),
               object_id=np.full((H, W), 0xA5A5A5A5, np.uint32))
    fr = rr_frame(out["rgba"].ctypes.data, out["normal"].ctypes.data, out["depth"].ctypes.data, out["object_id"].ctypes.data)
    return out, fr


def _setup(samples=2):
    fs = load_scene("spheres_room")
    return fs, camera_for(fs, W, H).c_struct(), make_config(samples=samples, monte_carlo=True, seed=6)


def _tiles(ds, cam, cfg, fr, n_passes, on_pass, cancel=None):
    L = capi.lib()
    cb = capi.PASS_FN(on_pass)
    return L.rr_render_progressive_tiles(ds._h, C.byref(cam), C.byref(cfg), None, C.byref(fr), n_passes, cb, None,
                                         C.byref(cancel) if cancel is not None else None)


def _zero(a):
    return not np.ascontiguousarray(a).view(np.uint8).any()


def test_tiles_cancelled_before_the_first_pass_leave_zero_buffers(hip):
    """A cancel flag already set returned before the first copy: `out` kept whatever the caller had in it."""
    fs, cam, cfg = _setup()
    calls = []
    with hip.DeviceScene(fs, 0) as ds:
        out, fr = _sentinel_frame()
        cancel = C.c_int(1)
        rc = _tiles(ds, cam, cfg, fr, 4, lambda u, d, t: calls.append(d) or 0, cancel)
        assert rc == -6, hip.lib().rr_last_error()
        assert not calls
        for k in ("rgba", "normal", "depth", "object_id"):
            assert _zero(out[k]), k


@pytest.mark.parametrize("stop_after", [0, 2])
def test_tiles_stopped_after_a_pass_hold_exactly_the_finished_tiles(hip, stop_after):
    fs, cam, cfg = _setup()
    P = 5
    with hip.DeviceScene(fs, 0) as ds:
        ref = ds.render(cam, cfg)
        out, fr = _sentinel_frame()
        calls = []

        def on_pass(user, done, total):
            calls.append(done)
            return 1 if len(calls) == stop_after + 1 else 0
        rc = _tiles(ds, cam, cfg, fr, P, on_pass)
        assert rc == -6 and len(calls) == stop_after + 1
        covered = np.zeros((H, W), bool)
        for k in range(stop_after + 1):
            xy = region_pixels(W, H, 32, 8, P, k)
            covered[xy[:, 1], xy[:, 0]] = True
        assert calls[-1] == int(covered.sum()) * cfg.samples
        for k in ("rgba", "normal", "depth", "object_id"):
            a, b = np.ascontiguousarray(out[k]), np.ascontiguousarray(ref[k])
            if a.dtype == np.float32:
                a, b = a.view(np.uint32), b.view(np.uint32)
            assert np.array_equal(a[covered], b[covered]), k    # the finished tiles: rr_render's pixels
            assert _zero(a[~covered]), k                          # the rest: zero


def reentry_child(tiles: bool):
    """The body of the re-entry test, in a child process: a regression of the in-pass marker is a self-deadlock on the scene's lock,
    which the parent turns into a failure by its time limit.  Raises (exit status 1) on a wrong answer."""
    fs, cam, cfg = _setup(samples=4)   # rr_render_progressive: 4 passes of one sample slice each
    L = capi.lib()
    with capi.DeviceScene(fs, 0) as ds:
        ref = ds.render(cam, cfg)
        ref_stats = ds.stats()
        seen = []

        def on_pass(user, done, total):
            st = rr_frame_stats()
            rc_stats = L.rr_scene_last_stats(ds._h, C.byref(st))
            inner = np.zeros((H, W, 4), np.uint8)
            ifr = rr_frame(inner.ctypes.data, None, None, None)
            rc_frame = L.rr_render(ds._h, C.byref(cam), C.byref(cfg), None, C.byref(ifr), None)
            seen.append((done, rc_stats, st.primary_rays, rc_frame, L.rr_last_error().decode(), bool(inner.any())))
            return 0
        out, fr = _sentinel_frame()
        cb = capi.PASS_FN(on_pass)
        fn = L.rr_render_progressive_tiles if tiles else L.rr_render_progressive
        rc = fn(ds._h, C.byref(cam), C.byref(cfg), None, C.byref(fr), 4, cb, None, None)
        assert rc == 0, L.rr_last_error()
        assert len(seen) >= 2
        for done, rc_stats, primary, rc_frame, msg, drawn in seen:
            assert rc_stats == 0 and primary == done, (done, primary)
            assert rc_frame == -1 and "re-entry" in msg and not drawn, (rc_frame, msg)
        assert_frames_identical(out, ref, "the progressive frame")
        st = ds.stats()
        for k in ("primary_rays", "secondary_rays", "shadow_rays", "shaded_hits"):
            assert st[k] == ref_stats[k], k
    print("REENTRY_OK", len(seen))


@pytest.mark.parametrize("tiles", [False, True])
def test_on_pass_may_read_its_scene_stats_and_is_refused_a_frame(hip, tiles):
    """Both progressive entry points held the scene's lock while they called on_pass: rr_scene_last_stats on the same scene, the
    natural way to show progress, deadlocked.  Run in a child process with a time limit, so that a deadlock fails the test."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + \
          ["-c", f"import tests.test_gpu_progressive as t; t.reentry_child({tiles})"]
    try:
        r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        pytest.fail("the progressive frame did not finish within 120 s: a call from on_pass deadlocked on the scene's lock")
    assert r.returncode == 0 and "REENTRY_OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
