"""What the shadow-query tests share (tests/test_gpu_shadow_rays.py, test_gpu_shadow_rays_cpp.py, test_shadow_rays_host.py):
the shadow rays the oracle traced while rendering a window, the limit classes built from the oracle's own toi, and the
expected record of rr_trace_shadow_rays for a ray and a limit.  No GPU is needed here.

The expected value, everywhere:
    occ = found & ~(toi > L)        # L = +inf for the NULL form; numpy's NaN compare is False, as the reference's
    if occ: item, face and the toi BITS equal the oracle's (NaN matches NaN)
    else:   occluded == 0, item == -1
"""
from __future__ import annotations

import functools
import os

import numpy as np

from rustray_amd.flat import RR_LIGHT_DIRECTIONAL, FlatScene, make_config
from tests.helpers import GOLDEN, camera_for, load_scene

FIXED_CLASSES = ("none", "t", "below_t", "half_t", "two_t", "zero", "1e30")


def shadow_log(oracle, fs, cam, cfg, window, cap=1 << 18):
    """The shadow `trace` calls of an oracle render of `window`, in call order: dict(origin, dir, depth, found, item, face, toi)."""
    with oracle.ray_log(cap) as log:
        oracle.render(fs.c_struct(), cam, cfg, window=window, n_threads=1)
        rays = log.rays()
    assert len(rays["depth"]) < cap, "ray log full"
    m = rays["for_shadow"]
    return {k: v[m] for k, v in rays.items() if k != "for_shadow"}


def limit_classes(fs, rays):
    """name -> per-ray limits (float32 array, or None = the NULL form).  t = the oracle's toi where found and finite, else 1.
    One class per point or spot light: |light.pos - origin| in float32; a ray whose origin is not finite has no such distance
    (the call refuses NaN), and takes +inf there: no limit for that ray."""
    toi = rays["toi"]
    t = np.where(rays["found"] & np.isfinite(toi), toi, np.float32(1.0)).astype(np.float32)
    out = {"none": None, "t": t, "below_t": np.nextafter(t, np.float32(0.0)), "half_t": np.float32(0.5) * t, "two_t": np.float32(2.0) * t,
           "zero": np.zeros_like(t), "1e30": np.full_like(t, np.float32(1e30))}
    for k, l in enumerate(fs.lights):
        if l.light_type == RR_LIGHT_DIRECTIONAL:
            continue
        diff = (np.asarray(l.pos, np.float32)[None, :] - rays["origin"]).astype(np.float32)
        dist = np.sqrt((diff * diff).sum(axis=1, dtype=np.float32)).astype(np.float32)
        out[f"light{k}"] = np.where(np.isfinite(dist), dist, np.float32(np.inf)).astype(np.float32)
    return out


def expected_occluded(rays, limit):
    L = np.float32(np.inf) if limit is None else limit
    with np.errstate(invalid="ignore"):
        return rays["found"] & ~(rays["toi"] > L)


def mismatches(got, rays, limit):
    """Indices of the rays whose record (occluded, item, face, toi) differs from the expected one."""
    occ, item, face, toi = got
    exp = expected_occluded(rays, limit)
    same_toi = (toi.view(np.uint32) == rays["toi"].view(np.uint32)) | (np.isnan(toi) & np.isnan(rays["toi"]))
    ok_occ = exp & occ & (item == rays["item"]) & (face == rays["face"]) & same_toi
    ok_lit = ~exp & ~occ & (item == -1) & (face == 0) & (toi.view(np.uint32) == 0)
    return np.flatnonzero(~(ok_occ | ok_lit))


def describe(fs_name, rays, limit, idx, got):
    i = int(idx[0])
    L = None if limit is None else float(limit[i])
    return (f"{fs_name}: {len(idx)} of {len(rays['toi'])} rays differ; first: ray {i} origin {rays['origin'][i].tolist()} dir {rays['dir'][i].tolist()} "
            f"depth {int(rays['depth'][i])} limit {L!r}: oracle found {bool(rays['found'][i])} item {int(rays['item'][i])} face {int(rays['face'][i])} "
            f"toi {float(rays['toi'][i])!r}, got occluded {bool(got[0][i])} item {int(got[1][i])} face {int(got[2][i])} toi {float(got[3][i])!r}")


def by_depth(rays):
    """(depth, index array) for every depth in the log."""
    return [(int(d), np.flatnonzero(rays["depth"] == d)) for d in sorted(set(rays["depth"].tolist()))]


def subset(rays, idx):
    return {k: v[idx] for k, v in rays.items()}


# ---- the logged cases (each rendered once per process)

@functools.lru_cache(maxsize=None)
def _spheres_room(oracle):
    fs = load_scene("spheres_room")
    cam = camera_for(fs, 96, 64).c_struct()
    cfg = make_config(samples=2, monte_carlo=True, seed=3, max_recursion=4)
    return fs, shadow_log(oracle, fs, cam, cfg, (24, 16, 72, 48))


def spheres_room_case(oracle):
    """spheres_room 96x64, window (24,16,72,48), 2 samples, Monte Carlo, seed 3, max_recursion 4: 109 248 shadow rays at depths 1-5."""
    return _spheres_room(oracle)


@functools.lru_cache(maxsize=None)
def _monkey(oracle):
    fs = load_scene("monkey")
    cam = camera_for(fs, 80, 60).c_struct()
    cfg = make_config(samples=1, monte_carlo=False, seed=0, max_recursion=3)
    return fs, shadow_log(oracle, fs, cam, cfg, (20, 10, 60, 50))


def monkey_case(oracle):
    """monkey 80x60, window (20,10,60,50), 1 sample, max_recursion 3: 1 902 shadow rays, 1 467 found."""
    return _monkey(oracle)


@functools.lru_cache(maxsize=None)
def _corner(oracle, name):
    from tests import corner_scenes
    fs = corner_scenes.builders()[name]()
    cam = camera_for(fs, 48, 36).c_struct()
    cfg = make_config(samples=1, monte_carlo=False, seed=0, max_recursion=3)
    return fs, shadow_log(oracle, fs, cam, cfg, None)


def corner_case(oracle, name):
    """A scene of tests/corner_scenes.builders() at 48x36, one sample."""
    return _corner(oracle, name)


@functools.lru_cache(maxsize=None)
def _fuzz_6601(oracle):
    fs = FlatScene.load(os.path.join(GOLDEN, "fuzz_6601.npz"))
    w, h = fs.meta["wh"]
    cam = camera_for(fs, w, h).c_struct()
    cfg = make_config(**fs.meta["kw"])
    return fs, shadow_log(oracle, fs, cam, cfg, None, cap=1 << 20)


def fuzz_6601_case(oracle):
    """tests/golden/fuzz_6601.npz with its own meta: one shadow ray has a NaN origin, found with a NaN toi."""
    return _fuzz_6601(oracle)
