"""Hand-made frames of rr_radiance records for the denoiser's tests (tests/test_denoise_host.py, tests/test_denoise_range_host.py,
tests/test_gpu_denoise.py, tests/test_gpu_denoise_range.py): the inputs only, made once per size and never changed by a test."""
import functools

import numpy as np

F = np.float32


def pack(color, depth, normal, ids):
    """(n, 8) float32 records of (n, 3) colours, (n,) depths, (n, 3) normals and (n,) uint32 ids."""
    n = len(depth)
    rec = np.zeros((n, 8), F)
    rec[:, 0:3], rec[:, 3], rec[:, 4:7] = color, depth, normal
    rec[:, 7] = np.asarray(ids, np.uint32).view(F)
    return rec


@functools.lru_cache(maxsize=None)
def quality_frame():
    """The 64x48 frame of the quality check: two ids split by a diagonal, a normal per id, a sloped depth, a colour ramp; the halves are
    the truth plus Gaussian noise of sigma 0.1 (default_rng(1)), the records their mean.  -> (truth (n, 3), records, halves)."""
    W, H = 64, 48
    y, x = np.mgrid[0:H, 0:W]
    x, y = x.reshape(-1), y.reshape(-1)
    right = (x * H > y * W)
    ids = np.where(right, 7, 3).astype(np.uint32)
    normal = np.where(right[:, None], np.array([0.0, 0.6, 0.8], F), np.array([0.0, 0.0, 1.0], F)).astype(F)
    depth = (F(4) + F(0.02) * x.astype(F) + F(0.01) * y.astype(F) + np.where(right, F(1.5), F(0))).astype(F)
    ramp = (F(0.1) + F(0.8) * x.astype(F) / F(W - 1)).astype(F)
    truth = np.stack([ramp, (ramp * F(0.5) + F(0.2)).astype(F), np.where(right, F(0.7), F(0.3)).astype(F)], axis=1).astype(F)
    rng = np.random.default_rng(1)
    halves = np.zeros((W * H, 2, 8), F)
    for h in range(2):
        halves[:, h] = pack((truth + rng.normal(0.0, 0.1, truth.shape)).astype(F), depth, normal, ids)
    color = ((halves[:, 0, 0:3] + halves[:, 1, 0:3]) * F(0.5)).astype(F)
    records = pack(color, depth, normal, ids)
    for a in (truth, records, halves):
        a.setflags(write=False)
    return truth, records, halves


@functools.lru_cache(maxsize=None)
def random_frame(W: int, H: int, seed: int = 5, bad: bool = True):
    """A W x H frame of 5 ids in irregular patches, unit normals, depths 1 .. 9, colours in [0, 2^10] (most below 2), halves around them,
    and an albedo with zeros, tiny values and ones.  With `bad`: some NaN / inf colours, some non-finite halves, some all-miss pixels
    (NaN normals, id 0, depth 0).  -> (records (n, 8), halves (n, 2, 8), albedo (n, 3))."""
    rng = np.random.default_rng(seed)
    n = W * H
    bad = bad and n >= 64           # (a tiny frame has no room for them)
    y, x = np.mgrid[0:H, 0:W]
    x, y = x.reshape(-1), y.reshape(-1)
    ids = (1 + ((x // 5 + 2 * (y // 4) + (x * y) // 23) % 5)).astype(np.uint32)
    nrm = rng.normal(size=(5, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F)
    normal = (nrm[ids - 1] + rng.normal(0, 0.05, (n, 3))).astype(F)
    normal = (normal / np.linalg.norm(normal, axis=1, keepdims=True).astype(F)).astype(F)
    depth = (F(1) + ids.astype(F) * F(1.5) + rng.random(n).astype(F) * F(0.5)).astype(F)
    base = rng.random((n, 3)).astype(F) * F(2)
    base[rng.random(n) < 0.02] *= F(400)          # a few bright pixels, still below 2^10
    noise = (rng.random((n, 3)).astype(F) - F(0.5)) * F(0.4)
    a = np.clip(base + noise, 0, 1023).astype(F)
    b = np.clip(base - noise, 0, 1023).astype(F)
    color = ((a + b) * F(0.5)).astype(F)
    albedo = (F(0.05) + rng.random((n, 3)).astype(F)).astype(F)
    albedo[rng.random(n) < 0.1] = 0
    albedo[rng.random(n) < 0.05, 1] = F(2.0 ** -10)       # not above the limit: left as it is
    albedo[rng.random(n) < 0.05, 2] = F(2.0 ** -9)
    if bad:
        k = rng.permutation(n)
        color[k[0:3], 0] = np.nan
        color[k[3:5], 2] = np.inf
        color[k[5], 1] = -np.inf
        a[k[6:9], 1] = np.nan                       # a non-finite half under a finite record: no variance seed there
        b[k[9], 0] = np.inf
        miss = k[10:10 + max(3, n // 20)]
        ids[miss], depth[miss], normal[miss] = 0, 0, np.nan
        albedo[k[30 % n], 0] = np.nan
    records = pack(color, depth, normal, ids)
    halves = np.zeros((n, 2, 8), F)
    halves[:, 0], halves[:, 1] = pack(a, depth, normal, ids), pack(b, depth, normal, ids)
    for arr in (records, halves, albedo):
        arr.setflags(write=False)
    return records, halves, albedo


RANGE_KINDS = ("colour_range", "colour_big", "colour_neg", "depth_range", "normal_zero", "normal_short", "normal_huge", "normal_flip",
               "var_zero", "var_tiny", "albedo_range", "mixed")
EXTRA_KINDS = ("colour_bands", "demod_overflow")


def _log_uniform(rng, lo, hi, shape):
    """2^e, e uniform in [lo, hi), rounded to float32 (2^-149 is the smallest subnormal: nothing rounds to 0)."""
    return np.exp2(rng.uniform(lo, hi, shape)).astype(F)


@functools.lru_cache(maxsize=None)
def range_frame(W: int, H: int, kind: str, seed: int = 11):
    """A plain W x H frame -- 3 ids in patches, the unit normal (0, 0.6, 0.8), depth 3 + 0.01 x, colours in [0, 2) with halves +-0.2 around
    them, an albedo in [0.25, 1.25), nothing non-finite -- with ONE thing taken to the ends of the float range (RANGE_KINDS):
      colour_range  colours log-uniform in 2^-149 .. 2^127, halves at +-25 %.  Above 2^65 or so a squared luminance difference overflows
                    to a +inf variance; a pixel of finite variance then meets such a tap at a weight whose square underflows, and
                    (w*w) * var_q = 0 * inf is a NaN variance (the header names it): with halves this kind generates NaN VARIANCES,
                    never a NaN colour
      colour_big    colours log-uniform in 2^100 .. 2^127.9, halves at +-1 %; the record is the float32 mean of its halves, whose sum
                    overflows above 2^127: those colours are inf and pass through
      colour_neg    colours +-2^-20 .. 2^20, half of them negative, halves at +-20 %
      depth_range   depths log-uniform in 2^-149 .. 2^127, a fifth negative
      normal_zero   10 % of the normals (0, 0, 0)           normal_short  every normal halved
      normal_huge   10 % of the normals scaled by 1e20      normal_flip   30 % of the normals negated
      var_zero      both halves equal to the record         var_tiny      halves at +-2^-23 relative
      albedo_range  albedo log-uniform in 2^-149 .. 2^127
      mixed         colour_range (the whole range in every id) + depth_range + normal_zero + albedo_range (on 3 % of the pixels, and
                    nowhere where colour / albedo would overflow), and the NaN / inf colours, non-finite halves, all-miss pixels and
                    NaN albedo of random_frame(bad=True)
    and two kinds of this suite's own (EXTRA_KINDS):
      colour_bands    colour_range with one band of the range per id -- 2^-149 .. 2^-60, 2^-60 .. 2^30 and 2^66 .. 2^127, where every
                      variance is +inf -- so that no NaN is generated and variances, too, are held to bits
      demod_overflow  where the header says "keep c_k / a_k finite": 12 % of the pixels of id 1 have an albedo of 2^-9 under a colour of
                      2^120 (record and both halves overflow at demodulation: an inf working colour that is a tap, and a NaN variance
                      seed, lum(inf) - lum(inf)) or of 2^118.8 (only the larger half overflows: a +inf seed)
    -> (records (n, 8), halves (n, 2, 8), albedo (n, 3))."""
    if kind not in RANGE_KINDS + EXTRA_KINDS:
        raise ValueError(kind)
    rng = np.random.default_rng(seed)
    n = W * H
    has = lambda k: kind == k or (kind == "mixed" and k in ("colour_range", "depth_range", "normal_zero", "albedo_range"))
    y, x = np.mgrid[0:H, 0:W]
    x, y = x.reshape(-1), y.reshape(-1)
    ids = (1 + ((x // 6 + y // 4 + (x * y) // 29) % 3)).astype(np.uint32)
    normal = np.tile(np.array([0.0, 0.6, 0.8], F), (n, 1))
    depth = (F(3) + F(0.01) * x.astype(F)).astype(F)
    albedo = (F(0.25) + rng.random((n, 3)).astype(F)).astype(F)
    # every kind draws the same numbers in the same order: a kind differs from the plain frame in its one thing only
    base = rng.random((n, 3)).astype(F) * F(2)
    noise = (rng.random((n, 3)).astype(F) - F(0.5)) * F(0.4)
    sign = np.where(rng.random((n, 3)) < 0.5, F(-1), F(1)).astype(F)
    unit = rng.random((n, 3))
    wide, big, mid = np.exp2(-149 + 276 * unit).astype(F), _log_uniform(rng, 100, 127.9, (n, 3)), _log_uniform(rng, -20, 20, (n, 3))
    wide_z, neg_z = _log_uniform(rng, -149, 127, n), rng.random(n) < 0.2
    pick = rng.random(n)
    wide_a, pick_a = _log_uniform(rng, -149, 127, (n, 3)), rng.random(n)
    with np.errstate(over="ignore", invalid="ignore"):
        if kind == "colour_bands":
            # one band of the range per id (see the docstring), drawn from the same uniform numbers; one sign per pixel, so that the
            # luminances of the halves differ by a quarter of the colour's and nothing cancels
            lo, span = np.array([-149, -60, 66], np.float64)[ids - 1], np.array([89, 90, 61], np.float64)[ids - 1]
            banded = np.exp2(lo[:, None] + span[:, None] * unit).astype(F)
            a, b = banded * (F(1) + F(0.25) * sign[:, :1]), banded * (F(1) - F(0.25) * sign[:, :1])
        elif has("colour_range"):
            a, b = wide * (F(1) + F(0.25) * sign), wide * (F(1) - F(0.25) * sign)
        elif has("colour_big"):
            a, b = big * (F(1) + F(0.01) * sign), big * (F(1) - F(0.01) * sign)
        elif has("colour_neg"):
            a, b = (sign * mid) * F(1.2), (sign * mid) * F(0.8)
        elif has("var_tiny"):
            a, b = base * (F(1) + F(2.0 ** -23)), base * (F(1) - F(2.0 ** -23))
        else:
            a, b = base + noise, base - noise
        a, b = a.astype(F), b.astype(F)
        if kind == "demod_overflow":
            for lo, hi, c in ((0.0, 0.06, 2.0 ** 120), (0.06, 0.12, 2.0 ** 118.8)):
                at = (pick_a >= lo) & (pick_a < hi) & (ids == 1)
                a[at], b[at], albedo[at] = F(c) * F(1.25), F(c) * F(0.75), F(2.0 ** -9)
        color = ((a + b) * F(0.5)).astype(F)
    if has("var_zero"):
        a, b = color.copy(), color.copy()
    if has("depth_range"):
        depth = np.where(neg_z, -wide_z, wide_z).astype(F)
    if has("normal_zero"):
        normal[pick < 0.1] = 0
    if has("normal_short"):
        normal = (normal * F(0.5)).astype(F)
    if has("normal_huge"):
        normal[pick < 0.1] *= F(1e20)
    if has("normal_flip"):
        normal[pick < 0.3] *= F(-1)
    if has("albedo_range"):
        plain, albedo = albedo, wide_a.copy()
        if kind == "mixed":
            # a colour above 2^117 over an albedo below 1 overflows at demodulation, and that inf is a tap of its whole id region
            # (include/rustray_hip.h names the case): the frame keeps clear of it, or nothing else in it would be looked at
            with np.errstate(all="ignore"):
                big_c = np.maximum(np.maximum(np.abs(a), np.abs(b)), np.abs(color))
                over = (albedo > F(2.0 ** -10)) & ~np.isfinite(big_c / albedo)
            # and remodulation of a region's mean, which the largest colours dominate, by an albedo above 1 overflows: only 3 %
            # of the pixels get the wide albedo, so that fewer than 5 % of the finite pixels come out non-finite
            over |= (pick_a >= 0.03)[:, None]
            albedo[over] = plain[over]
            with np.errstate(all="ignore"):
                albedo[~np.isfinite(big_c / albedo)] = 1           # (the plain albedo can be below 1 as well)
    if kind == "mixed" and n >= 64:
        k = rng.permutation(n)
        color[k[0:3], 0] = np.nan
        color[k[3:5], 2] = np.inf
        color[k[5], 1] = -np.inf
        a[k[6:9], 1] = np.nan
        b[k[9], 0] = np.inf
        miss = k[10:10 + max(3, n // 20)]
        ids[miss], depth[miss], normal[miss] = 0, 0, np.nan
        albedo[k[30 % n], 0] = np.nan
    records = pack(color, depth, normal, ids)
    halves = np.zeros((n, 2, 8), F)
    halves[:, 0], halves[:, 1] = pack(a, depth, normal, ids), pack(b, depth, normal, ids)
    for arr in (records, halves, albedo):
        arr.setflags(write=False)
    return records, halves, albedo


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def differing_words(got, want):
    """Two float32 arrays word by word -> (words that differ and are not a NaN on both sides, words that are NaNs of other bits on both
    sides).  The second count is allowed only where the arithmetic itself generated the NaN: its sign and payload are unspecified."""
    g, w = np.ascontiguousarray(got).view(np.uint32).reshape(-1), np.ascontiguousarray(want).view(np.uint32).reshape(-1)
    assert g.shape == w.shape
    both_nan = np.isnan(g.view(F)) & np.isnan(w.view(F))
    return int(((g != w) & ~both_nan).sum()), int(((g != w) & both_nan).sum())
