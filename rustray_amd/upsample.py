"""The joint-bilateral upsampler of rr_upsample_records in numpy float32: the yardstick the device kernel and the host loop over
rustray_amd/csrc/rr_upsample.h are held to, bit for bit.

Every step is exact in binary32 in the order include/rustray_hip.h states: float32 products and sums one at a time (numpy does not
contract), one correctly rounded division at a time, no transcendentals.  The four taps of a pixel are four whole-frame gathers here; a
tap that is skipped adds nothing (np.add(..., where=taken)), so the sums are those of the per-pixel loop.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .denoise import EPS, FLT_MAX, F, albedo_used
from .flat import SURFACE_HIT_DTYPE

MISS_NORMAL_BITS = 0xFFC00000    # what rr_render_pixels writes into the normal of a pixel all of whose rays missed (the device's 0 / 0)


@dataclass
class UpsampleParams:
    """rr_upsample_params without its struct_size; the defaults are rr_upsample_default_params'."""
    normal_power_log2: int = 5
    sigma_depth: float = 0.05
    use_albedo: bool = True
    gamma_correction: bool = False

    def check(self):
        if not 0 <= int(self.normal_power_log2) <= 7:
            raise ValueError(f"normal_power_log2 {self.normal_power_log2} (0 .. 7)")
        v = float(self.sigma_depth)
        if not (v > 0.0 and np.isfinite(F(v))):
            raise ValueError("sigma_depth must be finite and above 0")


def guide_array(guide, n: int) -> np.ndarray:
    """n rr_surface_hit records as the structured array flat.SURFACE_HIT_DTYPE: a structured array, or (n, 32) float32 words."""
    g = np.ascontiguousarray(guide)
    if g.dtype != SURFACE_HIT_DTYPE:
        g = np.ascontiguousarray(g, F).reshape(n, 32).view(SURFACE_HIT_DTYPE)
    return g.reshape(n)


def make_guide(hit, object_id, distance, normal, base_color) -> np.ndarray:
    """Surface records that hold the five fields the upsampler reads (everything else zero), for hand-made frames."""
    n = len(hit)
    g = np.zeros(n, SURFACE_HIT_DTYPE)
    g["hit"], g["object_id"], g["distance"], g["normal"] = hit, object_id, distance, normal
    g["base_color"][:, 0:3] = base_color
    g["base_color"][:, 3] = 1
    return g


def position(full: int, low: int):
    """(x0 (full,) int64, fx (full,) float32): where the centres of `full` pixels lie among `low` pixels."""
    x = np.arange(full, dtype=np.int64).astype(F)
    u = ((x + F(0.5)) * F(low)) / F(full) - F(0.5)
    x0 = np.floor(u)
    return x0.astype(np.int64), (u - x0).astype(F)


def ratio(W: int, H: int, w: int, h: int):
    return max(F(W) / F(w), F(H) / F(h))


def _guide_fields(g, H, W):
    hit = (g["hit"] != 0).reshape(H, W)
    z, nrm = g["distance"].reshape(H, W), g["normal"].reshape(H, W, 3)
    valid = hit & np.isfinite(z) & np.isfinite(nrm).all(-1)
    return hit, valid, g["object_id"].reshape(H, W), z, nrm, g["base_color"][:, 0:3].reshape(H, W, 3)


def _demodulate(c, albedo):
    out = c.copy()
    np.divide(c, albedo, out=out, where=albedo_used(albedo))
    return out


def _taps(w, h, W, H):
    """The four taps of every full pixel, dy outer, dx inner: (inside (H, W) bool, qy (H, 1), qx (1, W) clipped into the frame, b (H, W))."""
    x0, fx = position(W, w)
    y0, fy = position(H, h)
    for dy in (0, 1):
        for dx in (0, 1):
            qx, qy = x0 + dx, y0 + dy
            inside = ((qy >= 0) & (qy < h))[:, None] & ((qx >= 0) & (qx < w))[None, :]
            b = ((fx if dx else F(1) - fx)[None, :] * (fy if dy else F(1) - fy)[:, None]).astype(F)
            yield inside, np.clip(qy, 0, h - 1)[:, None], np.clip(qx, 0, w - 1)[None, :], b


def _guide_out(records, g_full, n):
    """The guide fields of n output records (..., 8): the full guide's for a hit, the all-miss bits of a frame for a miss."""
    hit = g_full["hit"] != 0
    shape = (n,) + (1,) * (records.ndim - 2)
    records[..., 3] = np.where(hit, g_full["distance"], F(0)).reshape(shape)
    miss = np.uint32(MISS_NORMAL_BITS).view(F)
    records[..., 4:7] = np.where(hit[:, None], g_full["normal"], miss).reshape(shape + (3,))
    records[..., 7] = np.where(hit, g_full["object_id"], np.uint32(0)).astype(np.uint32).view(F).reshape(shape)


def _fallback(low_c, low_h, fin_q, w, h, W, H):
    """The bilinear mean of the taps inside the low frame whose colour is finite -> (colour (H, W, 3), halves (H, W, 2, 3) or None); three
    zeros where there is no such tap."""
    sum_c, sum_b = np.zeros((H, W, 3), F), np.zeros((H, W), F)
    sum_h = None if low_h is None else np.zeros((H, W, 2, 3), F)
    for inside, qy, qx, b in _taps(w, h, W, H):
        taken = inside & fin_q[qy, qx]
        np.add(sum_c, b[..., None] * low_c[qy, qx], out=sum_c, where=taken[..., None])
        if sum_h is not None:
            np.add(sum_h, b[..., None, None] * low_h[qy, qx], out=sum_h, where=taken[..., None, None])
        np.add(sum_b, b, out=sum_b, where=taken)
    ok = (sum_b > 0) & (sum_b <= FLT_MAX)
    col = np.zeros((H, W, 3), F)
    np.divide(sum_c, sum_b[..., None], out=col, where=ok[..., None])
    hv = None
    if sum_h is not None:
        hv = np.zeros((H, W, 2, 3), F)
        np.divide(sum_h, sum_b[..., None, None], out=hv, where=ok[..., None, None])
    return col, hv


def _low_arrays(low, halves_low, w, h):
    rec = np.ascontiguousarray(low, F).reshape(h, w, 8)
    hv = None if halves_low is None else np.ascontiguousarray(halves_low, F).reshape(h, w, 2, 8)
    return rec[..., 0:3], (None if hv is None else hv[..., 0:3]), np.isfinite(rec[..., 0:3]).all(-1)


def _albedo_plane(plane, n: int, what: str) -> np.ndarray:
    a = np.ascontiguousarray(plane, F)
    if a.size != 3 * n:
        raise ValueError(f"{what}: {a.size} floats for {n} pixels x 3")
    return a.reshape(n, 3)


def upsample_records(low, halves_low, guide_low, guide, w: int, h: int, W: int, H: int, params: UpsampleParams | None = None, *, albedo_low=None,
                     albedo=None) -> dict:
    """low: (w * h, 8) float32 rr_radiance records of the low frame in row-major order; halves_low: (w * h, 2, 8) in the layout of
    render_pixel_parts at n_parts = 2, or None; guide_low, guide: w * h and W * H rr_surface_hit records (flat.SURFACE_HIT_DTYPE, or
    (n, 32) float32).  albedo_low (w * h, 3) and albedo (W * H, 3), each or None (rr_upsample_albedo_records): the plane stands wherever
    the header reads the base_color[0 .. 2] of guide_low and of guide; with use_albedo off they are not read.  Returns dict(records
    (W * H, 8) float32, halves (W * H, 2, 8) or None, weight (W * H,) float32)."""
    prm = params or UpsampleParams()
    prm.check()
    w, h, W, H = int(w), int(h), int(W), int(H)
    if not (1 <= w <= W <= 65535 and 1 <= h <= H <= 65535):
        raise ValueError(f"a low frame of {w}x{h} for a frame of {W}x{H}")
    n = W * H
    g_low, g_full = guide_array(guide_low, w * h), guide_array(guide, n)
    sd, r = F(prm.sigma_depth), ratio(W, H, w, h)
    with np.errstate(all="ignore"):
        low_c, low_h, fin_q = _low_arrays(low, halves_low, w, h)
        hit_q, valid_q, id_q, z_q, n_q, a_q = _guide_fields(g_low, h, w)
        hit_p, valid_p, id_p, z_p, n_p, a_p = _guide_fields(g_full, H, W)
        if albedo_low is not None and prm.use_albedo:
            a_q = _albedo_plane(albedo_low, w * h, "albedo_low").reshape(h, w, 3)
        if albedo is not None and prm.use_albedo:
            a_p = _albedo_plane(albedo, n, "albedo").reshape(H, W, 3)
        sum_c, sum_w = np.zeros((H, W, 3), F), np.zeros((H, W), F)
        sum_h = None if low_h is None else np.zeros((H, W, 2, 3), F)
        demod = bool(prm.use_albedo) & hit_p
        for inside, qy, qx, b in _taps(w, h, W, H):
            taken = inside & fin_q[qy, qx] & (hit_q[qy, qx] == hit_p) & ~(hit_p & (id_q[qy, qx] != id_p)) & (valid_q[qy, qx] == valid_p)
            nq = n_q[qy, qx]
            cs = (n_p[..., 0] * nq[..., 0] + n_p[..., 1] * nq[..., 1]) + n_p[..., 2] * nq[..., 2]
            cs = np.where(cs > 0, cs, F(0))
            for _ in range(int(prm.normal_power_log2)):
                cs = cs * cs
            wg = b * cs
            t = np.abs(z_p - z_q[qy, qx]) / ((sd * np.abs(z_p)) * r + EPS)
            wg = wg / (F(1) + t * t)
            wt = np.where(valid_p, wg, b).astype(F)
            c = np.where(demod[..., None], _demodulate(low_c[qy, qx], a_q[qy, qx]), low_c[qy, qx])
            np.add(sum_c, wt[..., None] * c, out=sum_c, where=taken[..., None])
            if sum_h is not None:
                a2 = np.broadcast_to(a_q[qy, qx][..., None, :], sum_h.shape)
                ch = np.where(demod[..., None, None], _demodulate(low_h[qy, qx], a2), low_h[qy, qx])
                np.add(sum_h, wt[..., None, None] * ch, out=sum_h, where=taken[..., None, None])
            np.add(sum_w, wt, out=sum_w, where=taken)
        ok = (sum_w > 0) & (sum_w <= FLT_MAX)
        col, hv = _fallback(low_c, low_h, fin_q, w, h, W, H)
        guided = sum_c / sum_w[..., None]
        guided = np.where(demod[..., None] & albedo_used(a_p), guided * a_p, guided)
        col = np.where(ok[..., None], guided, col)
        if sum_h is not None:
            gh = sum_h / sum_w[..., None, None]
            a2 = np.broadcast_to(a_p[..., None, :], gh.shape)
            gh = np.where(demod[..., None, None] & albedo_used(a2), gh * a2, gh)
            hv = np.where(ok[..., None, None], gh, hv)
        weight = np.where(ok, sum_w, F(0)).astype(F)
    out = np.zeros((n, 8), F)
    out[:, 0:3] = col.reshape(n, 3)
    _guide_out(out, g_full, n)
    halves = None
    if hv is not None:
        halves = np.zeros((n, 2, 8), F)
        halves[:, :, 0:3] = hv.reshape(n, 2, 3)
        _guide_out(halves, g_full, n)
    return dict(records=out, halves=halves, weight=weight.reshape(n))


def bilinear_records(low, halves_low, guide, w: int, h: int, W: int, H: int) -> dict:
    """The fallback of upsample_records alone, on every pixel: the bilinear mean of the taps with a finite colour, no guide in the
    weights and no albedo; the guide fields are the full guide's all the same.  For comparisons.  Returns the dict of upsample_records,
    every weight 0."""
    w, h, W, H = int(w), int(h), int(W), int(H)
    n = W * H
    g_full = guide_array(guide, n)
    with np.errstate(all="ignore"):
        low_c, low_h, fin_q = _low_arrays(low, halves_low, w, h)
        col, hv = _fallback(low_c, low_h, fin_q, w, h, W, H)
    out = np.zeros((n, 8), F)
    out[:, 0:3] = col.reshape(n, 3)
    _guide_out(out, g_full, n)
    halves = None
    if hv is not None:
        halves = np.zeros((n, 2, 8), F)
        halves[:, :, 0:3] = hv.reshape(n, 2, 3)
        _guide_out(halves, g_full, n)
    return dict(records=out, halves=halves, weight=np.zeros(n, F))
