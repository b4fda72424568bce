"""Albedo planes for the upsampler's tests (tests/test_upsample_planes_host.py, tests/test_gpu_upsample_albedo.py): the inputs only, made
once per shape and never changed by a test.  The frames and guides are those of tests/upsample_cases.py."""
import functools

import numpy as np

from rustray_amd.upsample import make_guide
from tests.denoise_cases import F
from tests.upsample_cases import _centres, quality_case, random_case, records_of

PLANE_SETS = (("low", True, False), ("full", False, True), ("both", True, True))   # (name, albedo_low given, albedo given)


def _plane(rng, guide):
    """A plane for the pixels of `guide`: [0.05, 1.05); with 64 pixels or more a 0, a 2^-10, the float above 2^-10, a NaN, a +inf and a
    negative value at hit pixels that are known (the first six hits, channel by channel); NaN at every pixel that is not a hit."""
    n = len(guide)
    plane = (F(0.05) + rng.random((n, 3)).astype(F)).astype(F)
    hit = guide["hit"] != 0
    if n >= 64:
        at = np.flatnonzero(hit)[:6]
        assert len(at) == 6
        plane[at[0], :] = 0
        plane[at[1], 1] = F(2.0 ** -10)
        plane[at[2], 2] = np.nextafter(F(2.0 ** -10), F(1))
        plane[at[3], 0] = np.nan
        plane[at[4], 1] = np.inf
        plane[at[5], 2] = F(-0.25)
    plane[~hit] = np.nan
    return plane


@functools.lru_cache(maxsize=None)
def random_planes(W: int, H: int, w: int, h: int, seed: int = 11):
    """-> (albedo_low (w h, 3), albedo (W H, 3)) for random_case(W, H, w, h)."""
    _, _, guide_low, guide = random_case(W, H, w, h)
    rng = np.random.default_rng(seed)
    planes = _plane(rng, guide_low), _plane(rng, guide)
    for a in planes:
        a.setflags(write=False)
    return planes


def guide_with(guide, plane):
    """A copy of `guide` whose base_color[0 .. 2] is `plane` (None: the guide itself)."""
    if plane is None:
        return guide
    g = guide.copy()
    g["base_color"][:, 0:3] = plane
    return g


@functools.lru_cache(maxsize=None)
def box_quality_case():
    """quality_case's scene at 64x48 <- 32x24 as sub-samples see it: its ids, normals, depth, texture and shade; the colour and the albedo
    of a pixel are the mean over a 4x4 sub-grid per full pixel and an 8x8 sub-grid per low pixel (the same points of the unit square), in
    float64, then cast to float32; the guides hold the albedo at the pixel centres, as quality_case's do.  The truth is the full pixels'
    averaged colour.  -> (truth (n, 3), low (w h, 8), guide_low, guide, mean_albedo_low (w h, 3), mean_albedo (n, 3))."""
    W, H, w, h = 64, 48, 32, 24
    _, _, guide_low, guide = quality_case()

    def averaged(Wk, Hk, sub):
        u, v = _centres(Wk * sub, Hk * sub)
        right = u > 0.2 + 0.6 * v
        tex = 0.5 + 0.35 * np.cos(2 * np.pi * 13 * u) * np.cos(2 * np.pi * 9 * v)
        albedo = np.stack([tex, 0.8 * tex + 0.1, 1.0 - 0.7 * tex], axis=1)
        shade = np.where(right, 0.3 + 0.5 * u, 0.9 - 0.4 * v)
        color = albedo * shade[:, None]
        box = lambda a: a.reshape(Hk, sub, Wk, sub, 3).mean(axis=(1, 3)).reshape(Wk * Hk, 3)
        return box(color).astype(F), box(albedo).astype(F)

    truth, mean_albedo = averaged(W, H, 4)
    color_low, mean_albedo_low = averaged(w, h, 8)
    low = records_of(color_low, guide_low)
    out = (truth, low, guide_low, guide, mean_albedo_low, mean_albedo)
    for arr in out:
        arr.setflags(write=False)
    return out
