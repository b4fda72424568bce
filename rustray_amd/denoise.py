"""The variance-guided a-trous filter of rr_denoise_records in numpy float32: the yardstick the device kernels and the host loop over
rustray_amd/csrc/rr_denoise.h are held to, bit for bit.

Every step is exact in binary32 in the order include/rustray_hip.h states: float32 products and sums one at a time (numpy does not
contract), one correctly rounded division or square root at a time, no transcendentals.  The 25 taps of a pass are 25 whole-frame
array operations here; a tap that is skipped adds nothing (np.add(..., where=taken)), so the sums are those of the per-pixel loop.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

F = np.float32
EPS = F(2.0 ** -20)
ALBEDO_MIN = F(2.0 ** -10)
FLT_MAX = np.finfo(np.float32).max
SPLINE = (F(0.375), F(0.25), F(0.0625))      # K[|d|]
PREFILTER = (F(0.5), F(0.25))
MAX_ITERATIONS = 6


@dataclass
class DenoiseParams:
    """rr_denoise_params without its struct_size; the defaults are rr_denoise_default_params'."""
    iterations: int = 5
    normal_power_log2: int = 5
    sigma_depth: float = 0.05
    sigma_luminance: float = 4.0
    gamma_correction: bool = False

    def check(self):
        if not 1 <= int(self.iterations) <= MAX_ITERATIONS:
            raise ValueError(f"iterations {self.iterations} (1 .. {MAX_ITERATIONS})")
        if not 0 <= int(self.normal_power_log2) <= 7:
            raise ValueError(f"normal_power_log2 {self.normal_power_log2} (0 .. 7)")
        for name in ("sigma_depth", "sigma_luminance"):
            v = float(getattr(self, name))
            if not (v > 0.0 and np.isfinite(F(v))):
                raise ValueError(f"{name} must be finite and above 0")


def lum(c):
    """(0.2126f*r + 0.7152f*g) + 0.0722f*b of an (..., 3) float32 array."""
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def albedo_used(a):
    return (a > ALBEDO_MIN) & (a <= FLT_MAX)


def _demodulate(c, albedo):
    out = c.copy()
    np.divide(c, albedo, out=out, where=albedo_used(albedo))
    return out


def _window(n, d):
    """Destination and source slices of a shift by d along an axis of length n: dest[i] reads src[i + d]; None when empty."""
    lo, hi = max(0, -d), min(n, n - d)
    if lo >= hi:
        return None
    return slice(lo, hi), slice(lo + d, hi + d)


def _pass_ok(fin, sum_w):
    """Where a pass divides: fin_p and sum_w in (0, FLT_MAX].  A weightless pixel (sum_w 0, inf or NaN: a zero or short normal, a dot
    product that overflows) keeps its colour and variance of the pass's input for this pass."""
    return fin & (sum_w > 0) & (sum_w <= FLT_MAX)


def atrous_denoise(records, halves, albedo, width: int, height: int, params: DenoiseParams | None = None) -> dict:
    """records: (width * height, 8) float32 rr_radiance records in row-major order (column 7 holds the object id's bits); halves:
    (width * height, 2, 8) in the layout of render_pixel_parts at n_parts = 2, or None; albedo: (width * height, 3) or None.
    Returns dict(records (n, 8) float32: the filtered records, variance (n,) float32: the last variance)."""
    prm = params or DenoiseParams()
    prm.check()
    W, H = int(width), int(height)
    rec = np.ascontiguousarray(records, F).reshape(H, W, 8)
    hv = None if halves is None else np.ascontiguousarray(halves, F).reshape(H, W, 2, 8)
    al = None if albedo is None else np.ascontiguousarray(albedo, F).reshape(H, W, 3)
    sd, sl = F(prm.sigma_depth), F(prm.sigma_luminance)

    with np.errstate(all="ignore"):
        colour = rec[..., 0:3]
        fin = np.isfinite(colour).all(-1)
        valid = np.isfinite(rec[..., 3]) & np.isfinite(rec[..., 4:7]).all(-1)
        ids = rec[..., 7].view(np.uint32)
        nrm, z = rec[..., 4:7], rec[..., 3]

        # ---- prepare
        c = colour.copy()
        if al is not None:
            c = np.where(fin[..., None], _demodulate(colour, al), colour)
        var = np.zeros((H, W), F)
        if hv is not None:
            a, b = hv[..., 0, 0:3], hv[..., 1, 0:3]
            seeded = fin & np.isfinite(a).all(-1) & np.isfinite(b).all(-1)
            if al is not None:
                a, b = _demodulate(a, al), _demodulate(b, al)
            d = (lum(a) - lum(b)) * F(0.5)
            v = np.where(seeded, d * d, F(0))
            sum_v, sum_g = np.zeros((H, W), F), np.zeros((H, W), F)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    wy, wx = _window(H, dy), _window(W, dx)
                    if wy is None or wx is None:
                        continue
                    g = PREFILTER[abs(dx)] * PREFILTER[abs(dy)]
                    taken = fin[wy[1], wx[1]]
                    np.add(sum_v[wy[0], wx[0]], g * v[wy[1], wx[1]], out=sum_v[wy[0], wx[0]], where=taken)
                    np.add(sum_g[wy[0], wx[0]], g, out=sum_g[wy[0], wx[0]], where=taken)
            np.divide(sum_v, sum_g, out=var, where=fin)

        # ---- the passes
        for i in range(int(prm.iterations)):
            s = 1 << i
            lum_c, sdev = lum(c), np.sqrt(var)
            den_l = sl * sdev + EPS
            sum_c, sum_v, sum_w = np.zeros((H, W, 3), F), np.zeros((H, W), F), np.zeros((H, W), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    wy, wx = _window(H, dy * s), _window(W, dx * s)
                    if wy is None or wx is None:
                        continue
                    P, Q = (wy[0], wx[0]), (wy[1], wx[1])
                    taken = fin[P] & fin[Q] & (ids[Q] == ids[P]) & (valid[Q] == valid[P])
                    w0 = SPLINE[abs(dx)] * SPLINE[abs(dy)]
                    n_p, n_q = nrm[P], nrm[Q]
                    cs = (n_p[..., 0] * n_q[..., 0] + n_p[..., 1] * n_q[..., 1]) + n_p[..., 2] * n_q[..., 2]
                    cs = np.where(cs > 0, cs, F(0))
                    for _ in range(int(prm.normal_power_log2)):
                        cs = cs * cs
                    wg = w0 * cs
                    if dx or dy:
                        t = np.abs(z[P] - z[Q]) / ((sd * np.abs(z[P])) * F(s * max(abs(dx), abs(dy))) + EPS)
                        wg = wg / (F(1) + t * t)
                    w = np.where(valid[P], wg, w0).astype(F)
                    if hv is not None:
                        t = np.abs(lum_c[P] - lum_c[Q]) / den_l[P]
                        w = w / (F(1) + t * t)
                    np.add(sum_c[P], w[..., None] * c[Q], out=sum_c[P], where=taken[..., None])
                    np.add(sum_v[P], (w * w) * var[Q], out=sum_v[P], where=taken)
                    np.add(sum_w[P], w, out=sum_w[P], where=taken)
            c_next, var_next = c.copy(), var.copy()
            ok = _pass_ok(fin, sum_w)
            np.divide(sum_c, sum_w[..., None], out=c_next, where=ok[..., None])
            np.divide(sum_v, sum_w * sum_w, out=var_next, where=ok)
            c, var = c_next, var_next

        # ---- finish
        if al is not None:
            c = np.where(albedo_used(al), c * al, c)
        out = rec.copy()
        out[..., 0:3] = np.where(fin[..., None], c, colour)
    # (np.where on float32 keeps NaN payloads: the colour of a non-finite pixel is the input's bits)
    return dict(records=out.reshape(H * W, 8), variance=var.reshape(H * W).copy())


def atrous_denoise_split(records, halves, diffuse, diffuse_halves, albedo, width: int, height: int, params: DenoiseParams | None = None) -> dict:
    """The filter of rr_denoise_split_records: the albedo is applied to the direct diffuse part of the colour alone.  records, halves, albedo
    as atrous_denoise takes them; diffuse: (width * height, 3) float32 (render_pixel_split), diffuse_halves: (width * height, 2, 3) or None,
    exactly when halves is.  Two record sets share depth, normal and id with `records`: `rest` with the colour records.color - diffuse (one
    binary32 subtraction) and `direct` with the colour diffuse; the halves are split the same way.  The colour returned is
    atrous_denoise(rest, rest halves, None).color + atrous_denoise(direct, direct halves, albedo).color, one binary32 add; a pixel whose
    record colour is not finite keeps the record's colour.  Returns dict(records (n, 8) float32)."""
    n = int(width) * int(height)
    rec = np.ascontiguousarray(records, F).reshape(n, 8)
    dif = np.ascontiguousarray(diffuse, F).reshape(n, 3)
    if (halves is None) != (diffuse_halves is None):
        raise ValueError("halves and diffuse_halves are given together or not at all")
    with np.errstate(all="ignore"):
        rest, direct = rec.copy(), rec.copy()
        rest[:, 0:3] = rec[:, 0:3] - dif
        direct[:, 0:3] = dif
        rest_h = direct_h = None
        if halves is not None:
            hv = np.ascontiguousarray(halves, F).reshape(n, 2, 8)
            dh = np.ascontiguousarray(diffuse_halves, F).reshape(n, 2, 3)
            rest_h, direct_h = hv.copy(), hv.copy()
            rest_h[:, :, 0:3] = hv[:, :, 0:3] - dh
            direct_h[:, :, 0:3] = dh
        a = atrous_denoise(rest, rest_h, None, width, height, params)["records"]
        b = atrous_denoise(direct, direct_h, albedo, width, height, params)["records"]
        out = rec.copy()
        fin = np.isfinite(rec[:, 0:3]).all(-1)
        out[:, 0:3] = np.where(fin[:, None], a[:, 0:3] + b[:, 0:3], rec[:, 0:3])
    return dict(records=out)


def frame_bytes_linear(color) -> np.ndarray:
    """The frame's bytes of (n, 3) linear colours without the gamma curve: (uint8)(fminf(c, 1) * 255) in float32, alpha 255 (what
    rr_render_pixels documents for gamma_correction = 0; NaN -> 0 as the device's conversion gives it)."""
    c = np.asarray(color, F)
    with np.errstate(all="ignore"):
        v = np.where(c < F(1), c, F(1)) * F(255)   # fminf(NaN, 1) = 1
        v = np.where(np.isnan(c), F(255), v)
        b = np.clip(v, 0, 255).astype(np.uint8)
    return np.concatenate([b, np.full((len(b), 1), 255, np.uint8)], axis=1)
