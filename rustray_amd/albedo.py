"""The sum of rr_albedo_pixels in numpy: the yardstick of the frame's albedo averaged over its sub-samples.

include/rustray_hip.h states it: every term (the base colour at the first hit of one primary ray, 0 for a miss) is clamped to +-32768,
scaled by 2^24 and rounded to nearest-even by itself, the terms are added as integers, and the channel is
(float)(sum * 2^-24) / (float)S -- rr_radiance.color's own sum.  A NaN term adds 0 and makes the channel NaN; a +inf (-inf) term adds the
clamp and makes it +inf (-inf); both signs in one pixel and channel make it NaN."""
import numpy as np

FIX_SCALE = 16777216.0  # 2^24 (RR_FIX_SCALE)
FIX_CLAMP = 32768.0     # RR_FIX_CLAMP


def mean_albedo(base_color, samples: int) -> np.ndarray:
    """(n, S, 3) float32 terms a(p, s) -> (n, 3) float32, bit for bit what rr_albedo_pixels writes for them; `samples` must be S."""
    a = np.asarray(base_color, np.float32)
    if a.ndim != 3 or a.shape[2] != 3 or a.shape[1] != samples or samples < 1:
        raise ValueError(f"mean_albedo: terms of shape {a.shape} for {samples} samples, (n, {samples}, 3) wanted")
    nan = np.isnan(a)
    pinf, ninf = np.isposinf(a), np.isneginf(a)
    v = np.where(nan, np.float32(0.0), a)
    v = np.minimum(np.maximum(v, np.float32(-FIX_CLAMP)), np.float32(FIX_CLAMP))
    fix = np.rint(v * np.float32(FIX_SCALE)).astype(np.int64)  # (the product is exact in binary32: a power of two; rint = nearest-even)
    total = fix.sum(axis=1)
    s = (total.astype(np.float64) * (1.0 / FIX_SCALE)).astype(np.float32)
    any_nan, any_pinf, any_ninf = nan.any(axis=1), pinf.any(axis=1), ninf.any(axis=1)
    s = np.where(any_pinf, np.float32(np.inf), s)
    s = np.where(any_ninf, np.float32(-np.inf), s)
    s = np.where(any_nan | (any_pinf & any_ninf), np.float32(np.nan), s)
    with np.errstate(invalid="ignore"):
        return (s / np.float32(samples)).astype(np.float32)
