"""Hand-made frames and histories for the tests of rr_accumulate_records (tests/test_temporal_host.py, tests/test_gpu_temporal.py): the
inputs only, made once per size and never changed by a test."""
import functools
import math

import numpy as np

from rustray_amd.camera import Camera
from rustray_amd.temporal import AccumulateParams, previous_view
from tests.denoise_cases import F, pack, random_frame


def make_camera(W, H, eye=(0.3, 0.2, 1.0), direction=(0.1, -0.05, -1.0), fov_scale=1.0):
    c = Camera()
    c.fov = c.fov * fov_scale
    c.eye_pos, c.dir = np.array(eye, np.float64), np.array(direction, np.float64)
    c.init(W, H)
    return c


def static_view(cam):
    """prev_world_to_clip and prev_eye of a camera that did not move: the float64 inverse of the camera's own float32 inverses, rounded
    to float32 -- what a host that kept only rr_camera would form."""
    pi = np.asarray(cam.projection_inverse, F).astype(np.float64)
    vi = np.asarray(cam.view_inverse, F).astype(np.float64)
    return (np.linalg.inv(pi) @ np.linalg.inv(vi)).astype(F), vi[:3, 3].astype(F)


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def temporal_frame(W: int, H: int):
    """A W x H current frame (denoise_cases.random_frame: 5 ids in patches, depths 2.5 .. 9, NaN / inf colours, non-finite halves,
    misses with NaN normals) with one pixel of negative depth (its world point lies behind the previous eye: clip.w <= 0), and a history
    for it: the same surfaces with other colours (their own NaN / inf colours and non-finite half-history), depths off by up to 4 %,
    a few normals turned by more than normal_min allows, lengths 0 (one in ten) or 1 .. 40.  The previous view is yawed by about 1.3
    pixels, shifted, and narrower (fov x 0.85), so that taps fall off every edge of the frame; `motion` moves the pixels of id 3.
    -> dict(cam, records, halves, history, history_halves, history_length, motion, prev_world_to_clip, prev_eye)."""
    rng = np.random.default_rng(11)
    n = W * H
    records, halves, _ = random_frame(W, H)
    other, other_halves, _ = random_frame(W, H, seed=7)
    records, halves = records.copy(), halves.copy()
    behind = (H // 2) * W + W // 2
    for layer in (records, halves[:, 0], halves[:, 1]):
        layer[behind, 0:3], layer[behind, 3], layer[behind, 4:7] = F(0.5), F(-50), np.array([0, 0, 1], F)
    history, history_halves = records.copy(), halves.copy()
    history[:, 0:3], history_halves[:, :, 0:3] = other[:, 0:3], other_halves[:, :, 0:3]
    history[:, 3] = (records[:, 3] * (F(1) + (rng.random(n).astype(F) - F(0.5)) * F(0.08))).astype(F)
    turned = rng.random(n) < 0.08
    history[turned, 4:7] = np.array([0.6, 0.0, 0.8], F)
    history[rng.random(n) < 0.02, 3] = np.inf
    history[rng.random(n) < 0.02, 7] = np.uint32(77).view(F)
    history_length = np.where(rng.random(n) < 0.1, F(0), (F(1) + rng.random(n).astype(F) * F(39))).astype(F)
    cam = make_camera(W, H)
    pitch = 2.0 / W                                   # radians per pixel at the centre, fov 90 degrees
    a = 1.3 * pitch
    d = cam.dir / np.linalg.norm(cam.dir)
    prev = make_camera(W, H, eye=cam.eye_pos + np.array([0.02, -0.01, -0.05]), fov_scale=0.85,
                       direction=(d[0] * math.cos(a) - d[2] * math.sin(a), d[1], d[0] * math.sin(a) + d[2] * math.cos(a)))
    prev_world_to_clip, prev_eye = previous_view(prev)
    ids = records[:, 7].view(np.uint32)
    motion = np.zeros((n, 3), F)
    motion[ids == 3] = (rng.normal(0, 0.04, (int((ids == 3).sum()), 3))).astype(F)
    return _freeze(dict(cam=cam, records=records, halves=halves, history=history, history_halves=history_halves, history_length=history_length,
                        motion=motion, prev_world_to_clip=prev_world_to_clip, prev_eye=prev_eye))


def frame_params(case, **kw) -> AccumulateParams:
    return AccumulateParams(prev_world_to_clip=case["prev_world_to_clip"], prev_eye=case["prev_eye"], **kw)


@functools.lru_cache(maxsize=None)
def static_frames(W: int, H: int, count: int):
    """`count` frames of one static view: the guide of random_frame(W, H, bad=False) (5 ids, depths 2.5 .. 9) under `count` different
    colour sets in [0, 2), halves around them.  -> (cam, params of the static view, records (count, n, 8), halves (count, n, 2, 8))."""
    rng = np.random.default_rng(3)
    base, _, _ = random_frame(W, H, bad=False)
    n = W * H
    records, halves = np.zeros((count, n, 8), F), np.zeros((count, n, 2, 8), F)
    for k in range(count):
        c = rng.random((n, 3)).astype(F) * F(2)
        noise = (rng.random((n, 3)).astype(F) - F(0.5)) * F(0.25)
        records[k] = base
        records[k, :, 0:3] = c
        halves[k, :, 0], halves[k, :, 1] = base, base
        halves[k, :, 0, 0:3], halves[k, :, 1, 0:3] = c + noise, c - noise
    cam = make_camera(W, H)
    m, eye = static_view(cam)
    records.setflags(write=False)
    halves.setflags(write=False)
    return cam, AccumulateParams(prev_world_to_clip=m, prev_eye=eye), records, halves


@functools.lru_cache(maxsize=None)
def boundary_frames(W: int = 40, H: int = 12, at: int = 17, shift: int = 3):
    """Two frames of one static view, flat depth and normal: the boundary between id 3 (left) and id 9 lies at column `at` in the first
    and at `at + shift` in the second.  -> (cam, params, first records, second records)."""
    x = np.arange(W * H) % W
    n = W * H

    def frame(edge, level):
        ids = np.where(x < edge, 3, 9).astype(np.uint32)
        color = np.where((x < edge)[:, None], F(level), F(level * 0.5)) * np.ones((n, 3), F)
        return pack(color.astype(F), np.full(n, 4, F), np.tile(np.array([0, 0, 1], F), (n, 1)), ids)
    cam = make_camera(W, H)
    m, eye = static_view(cam)
    first, second = frame(at, 0.75), frame(at + shift, 0.25)
    first.setflags(write=False)
    second.setflags(write=False)
    return cam, AccumulateParams(prev_world_to_clip=m, prev_eye=eye), first, second
