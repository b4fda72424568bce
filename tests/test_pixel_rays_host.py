"""The pinhole ray of a pixel centre without a GPU: the host program over rustray_amd/csrc/rr_pixel_list.h (the functions k_pixel_rays applies
per lane, and the bound rr_surface_pixels pads the top level with before its first launch) against the numpy yardstick
pixel_rays.pixel_rays, bit for bit; temporal_world and temporal.world_positions, which both take their ray from there now, against what
they gave before; and the four-corner reach bound against the largest origin of every pixel, brute force.  The program is built with
AddressSanitizer + UBSan and run as it is: a plain host program with nothing preloaded."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from rustray_amd.flat import rr_camera
from rustray_amd.pixel_rays import pixel_rays
from rustray_amd.temporal import world_positions
from tests.helpers import ROOT, camera_for, load_scene

F = np.float32
FLAGS = ["-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
FRAMES = ((1, 1), (3, 2), (50, 38), (65535, 1))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("pixel_rays") / "pixel_rays_test")
    subprocess.check_call(["g++"] + FLAGS + ["-o", path, os.path.join(ROOT, "tests", "native", "pixel_rays_test.cpp")])
    return path


def scene_camera(width, height) -> rr_camera:
    return camera_for(load_scene("spheres"), width, height).c_struct()


def odd_camera(width, height) -> rr_camera:
    """A camera whose matrices hold a NaN and an infinity: every ray must pass through the arithmetic and nothing may trap."""
    cam = rr_camera.from_buffer_copy(scene_camera(width, height))
    cam.projection_inverse[5] = float("nan")
    cam.view_inverse[8] = float("inf")
    return cam


def matrices(cam):
    return np.array(cam.projection_inverse[:], F), np.array(cam.view_inverse[:], F)


def run(exe, tmp_path, cases):
    """cases: (width, height, mode, proj_inv (16,), view_inv (16,), depths or None) -> the program's output as bytes."""
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as fh:
        fh.write(struct.pack("<I", len(cases)))
        for w, h, mode, pi, vi, depth in cases:
            fh.write(struct.pack("<3I", w, h, mode) + np.asarray(pi, F).tobytes() + np.asarray(vi, F).tobytes())
            if depth is not None:
                fh.write(np.ascontiguousarray(depth, F).tobytes())
    out = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "pixel rays test OK" in out.stdout, out.stdout + out.stderr
    return open(dst, "rb").read()


def same_words(a, b) -> bool:
    """Equal bits, except that a word that is a NaN on both sides counts as equal (a NaN the arithmetic generated has no specified sign)."""
    a, b = np.ascontiguousarray(a, F).reshape(-1), np.ascontiguousarray(b, F).reshape(-1)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.parametrize("make", (scene_camera, odd_camera), ids=("scene", "nan_inf"))
@pytest.mark.parametrize("size", FRAMES)
def test_host_rays_equal_the_yardstick(exe, tmp_path, size, make):
    w, h = size
    cam = make(w, h)
    pi, vi = matrices(cam)
    first_last = w * h > 4096
    raw = run(exe, tmp_path, [(w, h, 1 if first_last else 0, pi, vi, None)])
    pixels = np.array([[0, 0], [w - 1, h - 1]]) if first_last else None
    o, d = pixel_rays(cam, pixels)
    n = len(o)
    assert len(raw) == 24 * n + 24
    got = np.frombuffer(raw[:24 * n], F).reshape(n, 6)
    assert same_words(got[:, :3], o) and same_words(got[:, 3:], d)
    if make is scene_camera:
        assert np.isfinite(got).all() and np.allclose(np.linalg.norm(d.astype(np.float64), axis=1), 1.0, atol=1e-6)
    else:
        assert not np.isfinite(got).all()          # the NaN and the infinity reached the rays


def test_pixel_rays_of_a_list_are_the_frames(exe):
    cam = scene_camera(50, 38)
    o, d = pixel_rays(cam)
    px = np.array([[49, 37], [0, 0], [7, 8], [7, 8], [13, 0]])
    lo, ld = pixel_rays(cam, px)
    at = px[:, 1] * 50 + px[:, 0]
    assert same_words(lo, o[at]) and same_words(ld, d[at])
    packed = (px[:, 0] | (px[:, 1] << 16)).astype(np.uint32)
    assert same_words(pixel_rays(cam, packed)[0], lo)


def _old_world_positions(records, cam):
    """temporal.world_positions as it stood before it took its ray from pixel_rays: the refactor's yardstick."""
    pi, vi = matrices(cam)
    W, H = int(cam.width), int(cam.height)
    rec = np.ascontiguousarray(records, F).reshape(H * W, 8)
    y, x = np.mgrid[0:H, 0:W]
    x_f, y_f = x.reshape(-1).astype(F), y.reshape(-1).astype(F)
    one, zero = F(1), F(0)
    row = lambda m, r, a, b, c, e: ((m[r] * a + m[4 + r] * b) + m[8 + r] * c) + m[12 + r] * e
    with np.errstate(all="ignore"):
        cx = ((x_f + F(0.5)) / F(W)) * F(2) - one
        cy = one - ((y_f + F(0.5)) / F(H)) * F(2)
        pp = [row(pi, r, cx, cy, F(-1), one) for r in range(3)]
        o = [row(vi, r, pp[0], pp[1], pp[2], one) for r in range(3)]
        d = np.stack([row(vi, r, pp[0], pp[1], pp[2], zero) for r in range(3)], axis=-1)
        length = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
        return np.stack([o[r] + (d[..., r] / length) * rec[:, 3] for r in range(3)], axis=-1).astype(F)


@pytest.mark.parametrize("make", (scene_camera, odd_camera), ids=("scene", "nan_inf"))
def test_world_positions_keep_their_bits(exe, tmp_path, make):
    """o + d * depth from pixel_rays == temporal.world_positions == what world_positions gave before the refactor == the host's
    temporal_world, on a 37x19 frame of random depths (some of them not finite)."""
    w, h = 37, 19
    cam = make(w, h)
    rng = np.random.default_rng(20)
    depth = rng.uniform(0.0, 40.0, w * h).astype(F)
    depth[5], depth[6], depth[7] = np.nan, np.inf, F(3e38)
    rec = np.zeros((w * h, 8), F)
    rec[:, 3] = depth
    o, d = pixel_rays(cam)
    with np.errstate(all="ignore"):
        mine = (o + d * depth[:, None]).astype(F)
    want = world_positions(rec, cam)
    assert same_words(mine, want) and same_words(want, _old_world_positions(rec, cam))
    pi, vi = matrices(cam)
    raw = run(exe, tmp_path, [(w, h, 2, pi, vi, depth)])
    assert same_words(np.frombuffer(raw, F).reshape(-1, 3), want)
    if make is scene_camera:
        assert np.isfinite(want[8:]).all()


def test_slot_order_walks_every_frame_once(exe, tmp_path):
    """pixel_of_block_slot against the plain loops (inside the program: exit 2 on the first difference) for widths and heights around the
    multiples of 8, a single row, a single column and the largest width."""
    pi, vi = matrices(scene_camera(8, 8))
    sizes = [(w, h) for w in (1, 7, 8, 9, 16, 17, 70) for h in (1, 7, 8, 9, 41)] + [(65535, 1), (1, 65535), (4099, 9)]
    depth = {s: np.zeros(s[0] * s[1], F) for s in sizes}
    run(exe, tmp_path, [(w, h, 2, pi, vi, depth[(w, h)]) for w, h in sizes])


def test_reach_bounds_every_origin(exe, tmp_path):
    """The bound rr_surface_pixels pads the top level with, from the camera alone: for 1000 random cameras and frame sizes it is >= the
    largest |origin| component over EVERY pixel (numpy, brute force), and it is not slack: within 1 % of it plus the rounding term."""
    rng = np.random.default_rng(355)
    cases, cams = [], []
    for k in range(1000):
        w, h = int(rng.integers(1, 48)), int(rng.integers(1, 48))
        scale = 10.0 ** rng.uniform(-2, 4, 2)
        pi = (rng.standard_normal(16) * scale[0]).astype(F)
        vi = (rng.standard_normal(16) * scale[1]).astype(F)
        if k % 7 == 0:                       # a proper pinhole camera far from the origin, as a frame would have
            base = scene_camera(w, h)
            pi, vi = matrices(base)
            vi[12:15] += (rng.standard_normal(3) * 1e4).astype(F)
        cam = rr_camera()
        cam.width, cam.height = w, h
        cam.projection_inverse[:] = [float(v) for v in pi]
        cam.view_inverse[:] = [float(v) for v in vi]
        cams.append(cam)
        cases.append((w, h, 3, pi, vi, None))
    raw = run(exe, tmp_path, cases)
    reach = np.frombuffer(raw, np.float64).reshape(1000, 3)
    assert np.isfinite(reach).all()
    tight = 0
    for cam, r in zip(cams, reach):
        o, _ = pixel_rays(cam)
        worst = np.abs(o.astype(np.float64)).max(axis=0)
        assert (r >= worst).all(), (int(cam.width), int(cam.height), r, worst)
        tight += int((r <= 1.05 * worst + 1e-30).all())
    assert tight > 900                       # (cancelling terms widen the rounding term; most cameras have none)
