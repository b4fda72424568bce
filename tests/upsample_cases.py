"""Hand-made low frames and guides for the upsampler's tests (tests/test_upsample_host.py, tests/test_gpu_upsample.py): the inputs only,
made once per shape and never changed by a test.  Both guides of a case sample ONE scene given over the unit square at their own pixel
centres, so the low guide agrees with the full one where the scene is smooth and disagrees along its edges, whatever the ratio."""
import functools

import numpy as np

from rustray_amd.upsample import make_guide
from tests.denoise_cases import F, pack

# (W, H, w, h): the shapes of the host test; the GPU test adds the last one
SHAPES = ((37, 19, 19, 10), (65, 17, 17, 5), (9, 1, 3, 1), (1, 1, 1, 1), (33, 9, 33, 9))
GPU_SHAPES = SHAPES + ((64, 48, 32, 24),)


def _centres(W, H):
    y, x = np.mgrid[0:H, 0:W]
    return ((x.reshape(-1) + 0.5) / W), ((y.reshape(-1) + 0.5) / H)


def _scene_ids(u, v):
    """5 ids in irregular patches over the unit square; 0 = nothing there (a disc of the background)."""
    ids = 1 + ((np.floor(u * 7) + 2 * np.floor(v * 5) + np.floor(u * v * 11)).astype(np.int64) % 5)
    ids[(u - 0.3) ** 2 + (v - 0.6) ** 2 < 0.02] = 0
    return ids.astype(np.uint32)


def _guide(rng, W, H, bad):
    u, v = _centres(W, H)
    n = W * H
    ids = _scene_ids(u, v)
    base_n = np.array([[0.0, 0.0, 1.0], [0.0, 0.6, 0.8], [0.6, 0.0, 0.8], [-0.48, 0.6, 0.64], [0.0, -0.8, 0.6]], F)
    normal = (base_n[np.maximum(ids, 1) - 1] + rng.normal(0, 0.05, (n, 3))).astype(F)
    normal = (normal / np.linalg.norm(normal, axis=1, keepdims=True).astype(F)).astype(F)
    depth = (F(1) + ids.astype(F) * F(1.5) + (u + 0.5 * v).astype(F) * F(0.5)).astype(F)
    albedo = (F(0.05) + rng.random((n, 3)).astype(F)).astype(F)
    hit = (ids != 0).astype(np.uint32)
    if bad:
        k = rng.permutation(np.flatnonzero(hit))
        hit[k[0:2]] = 0                              # a pixel of a surface that this guide alone missed
        normal[k[2], 1] = np.nan                     # a NaN normal on a hit: not valid, a tap of pixels that are not valid either
        albedo[k[3:6]] = 0
        albedo[k[6:8], 1] = F(2.0 ** -10)            # not above the limit: left as it is
        albedo[k[8], 0] = np.nan
    # a miss as rr_surface_pixels writes it: {0, 0xffffffff, 0, 0} and zeros
    g = make_guide(hit, np.where(hit != 0, ids, 0), np.where(hit != 0, depth, 0), np.where(hit[:, None] != 0, normal, 0), np.where(hit[:, None] != 0, albedo, 0))
    g["item_index"] = np.where(hit != 0, ids, 0xffffffff)
    return g


@functools.lru_cache(maxsize=None)
def random_case(W: int, H: int, w: int, h: int, seed: int = 7):
    """-> (low (w h, 8), halves_low (w h, 2, 8), guide_low (w h,), guide (W H,)): colours in [0, 2) with halves around them and, where the
    low frame has room for them (64 pixels), NaN and inf colours, a non-finite half under a finite colour, and in both guides pixels only
    one of them missed, a NaN normal on a hit and albedos of 0, 2^-10 and NaN."""
    rng = np.random.default_rng(seed)
    guide_low, guide = _guide(rng, w, h, w * h >= 64), _guide(rng, W, H, W * H >= 64)
    n = w * h
    base = rng.random((n, 3)).astype(F) * F(2)
    noise = (rng.random((n, 3)).astype(F) - F(0.5)) * F(0.4)
    a, b = (base + noise).astype(F), (base - noise).astype(F)
    color = ((a + b) * F(0.5)).astype(F)
    if n >= 64:
        k = rng.permutation(n)
        color[k[0:3], 0] = np.nan
        color[k[3:5], 2] = np.inf
        color[k[5], 1] = -np.inf
        a[k[6:8], 1] = np.nan
        b[k[8], 0] = np.inf
    depth, normal, ids = guide_low["distance"], guide_low["normal"], guide_low["object_id"]
    low = pack(color, depth, normal, ids)
    halves = np.zeros((n, 2, 8), F)
    halves[:, 0], halves[:, 1] = pack(a, depth, normal, ids), pack(b, depth, normal, ids)
    for arr in (low, halves, guide_low, guide):
        arr.setflags(write=False)
    return low, halves, guide_low, guide


def flat_guide(W, H, ids=4, normal=(0.0, 0.0, 1.0), depth=3.0, albedo=0.5):
    n = W * H
    return make_guide(np.ones(n, np.uint32), np.broadcast_to(np.asarray(ids, np.uint32), (n,)), np.full(n, depth, F), np.tile(np.array(normal, F), (n, 1)),
                      np.full((n, 3), albedo, F))


def records_of(color, guide):
    return pack(color, guide["distance"], guide["normal"], guide["object_id"])


@functools.lru_cache(maxsize=None)
def quality_case():
    """64x48 <- 32x24: two ids split by a diagonal, a normal per id, a slanted depth ramp; the colour is a textured albedo (a product of
    two cosines, about five full pixels a period) times a smooth shade per id.  The truth is the colour at the full centres, the low frame
    the colour at the low centres; each guide holds the albedo at its own centres.  -> (truth (n, 3), low, guide_low, guide)."""
    W, H, w, h = 64, 48, 32, 24

    def sample(Wk, Hk):
        u, v = _centres(Wk, Hk)
        right = u > 0.2 + 0.6 * v
        ids = np.where(right, 7, 3).astype(np.uint32)
        normal = np.where(right[:, None], np.array([0.0, 0.6, 0.8], F), np.array([0.0, 0.0, 1.0], F)).astype(F)
        depth = (4.0 + 1.3 * u + 0.6 * v + np.where(right, 1.5, 0.0)).astype(F)
        tex = 0.5 + 0.35 * np.cos(2 * np.pi * 13 * u) * np.cos(2 * np.pi * 9 * v)
        albedo = np.stack([tex, 0.8 * tex + 0.1, 1.0 - 0.7 * tex], axis=1).astype(F)
        shade = np.where(right, 0.3 + 0.5 * u, 0.9 - 0.4 * v)
        color = (albedo.astype(np.float64) * shade[:, None]).astype(F)
        return color, make_guide(np.ones(Wk * Hk, np.uint32), ids, depth, normal, albedo)

    truth, guide = sample(W, H)
    color_low, guide_low = sample(w, h)
    low = records_of(color_low, guide_low)
    for arr in (truth, low, guide_low, guide):
        arr.setflags(write=False)
    return truth, low, guide_low, guide
