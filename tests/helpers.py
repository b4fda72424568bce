"""Shared helpers for the test suite: fixture scenes, cameras, comparisons."""
from __future__ import annotations

import os

import numpy as np

from rustray_amd.camera import Camera
from rustray_amd.flat import FlatScene, make_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "scenes")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def host_api_source() -> str:
    """The text of the library's host side: rustray_amd/csrc/rr_api.hip and every project header under csrc that its `#include "..."`
    lines reach, each once, in include order -- without rr_kernels.hip and the headers the kernels are made of (what rr_kernels.hip
    includes itself).  The tests that read the source text read it through here, so a layer file cannot drop out of their sight."""
    import re
    csrc = os.path.join(ROOT, "rustray_amd", "csrc")

    def walk(name, seen, texts):
        if name in seen or os.path.dirname(name) or not os.path.exists(os.path.join(csrc, name)):
            return   # seen already, or outside csrc (../../include/rustray_hip.h)
        seen.add(name)
        with open(os.path.join(csrc, name)) as fh:
            text = fh.read()
        texts.append(text)
        for inc in re.findall(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', text, re.M):
            walk(inc, seen, texts)

    kernel_side, host = set(), []
    walk("rr_kernels.hip", kernel_side, [])
    walk("rr_api.hip", set(kernel_side), host)
    return "\n".join(host)


def n_params(arglist: str) -> int:
    """The number of parameters in the text between a declaration's parentheses.  The callback type of rr_render_progressive has
    parameters of its own: nested parentheses are folded away before the commas are counted."""
    depth, flat = 0, []
    for ch in arglist:
        if ch == "(":
            depth += 1
        elif ch == ")":
            depth -= 1
        elif depth == 0:
            flat.append(ch)
    t = "".join(flat).strip()
    return 0 if t in ("", "void") else t.count(",") + 1


def arglist_after(text: str, pos: int) -> str:
    """The text from `pos`, just behind an opening parenthesis, to the parenthesis that closes it."""
    depth, i = 1, pos
    while depth:
        depth += {"(": 1, ")": -1}.get(text[i], 0)
        i += 1
    return text[pos:i - 1]


def load_scene(name: str) -> FlatScene:
    return FlatScene.load(os.path.join(SCENES, name + ".npz"))


def camera_for(fs: FlatScene, width: int, height: int) -> Camera:
    st = dict(fs.meta["camera"])
    st["width"], st["height"] = width, height
    return Camera.from_state(st)


# ---------------------------------------------------------------------------------------------------------------------
# The quantisation band.  Device and oracle both map a pixel's linear mean c to a byte with
# q(c) = as_u8(255 * g(min(c, 1))), g the identity or pow(., f32(1/2.2)); q is monotone.  For the oracle's float64 mean m
# of its own per-sample f32 colours, a correct device byte lies in [q(m - e), q(m + e)], e = eps_rel * |m| + eps_abs,
# with q evaluated in float64 and its argument widened by BAND_ARG_SLACK for the f32 roundings of the mean, of 255 * c
# and powf's ulps.
# ---------------------------------------------------------------------------------------------------------------------
BAND_EPS_REL = 1e-5          # shading arithmetic in another order (factorised path weights): ~80 f32 ulps per term
BAND_EPS_ABS = 2.0 ** -20    # per-term rounding to the 2^-24 fixed point, summed over up to 32 terms per sample
BAND_EPS_REL_MAX = 1e-4      # the ceiling for a test that derives a wider band next to its call
BAND_EPS_ABS_MAX = 2.0 ** -16
BAND_ARG_SLACK = 1e-3        # LSB, on the argument of as_u8
D6_CLAMP = 32768.0           # colour terms are clamped to +-32768 before accumulation
INV_GAMMA = float(np.float32(1.0 / 2.2))
DEPTH_HALF_STEP = 2.0 ** -17  # half a 2^-16 step of the depth accumulator
NORMAL_TERM_ERR = 2.0 ** -25  # rounding of one normal component to the 2^-24 fixed point
NORMAL_MIN_NORM = 1e-3        # pixels whose mean normal is shorter are not judged (the direction is ill-conditioned)
U32 = 2.0 ** -24


def _g(c, gamma):
    """g(min(c, 1)) in float64; negative c maps to 0 (pow of a negative is NaN, and as_u8(NaN) = 0 too)."""
    c = np.minimum(np.asarray(c, np.float64), 1.0)
    return np.where(gamma, np.power(np.maximum(c, 0.0), INV_GAMMA), c)


def _g_inv(y, gamma):
    y = np.asarray(y, np.float64)
    return np.where(gamma, np.power(np.maximum(y, 0.0), 1.0 / INV_GAMMA), y)


def as_u8(x):
    """The f32 -> u8 cast of both implementations (NaN -> 0, saturating), on float64 arguments."""
    x = np.asarray(x, np.float64)
    return np.where(np.isnan(x), 0, np.clip(np.floor(np.nan_to_num(x, nan=0.0)), 0, 255)).astype(np.int32)


def band_bytes(m, gamma=False, eps_rel=BAND_EPS_REL, eps_abs=BAND_EPS_ABS):
    """(lo, hi): the bytes a channel of float64 mean m may take.  m finite."""
    m = np.asarray(m, np.float64)
    e = eps_rel * np.abs(m) + eps_abs
    return as_u8(_arg_lo(m - e, gamma)), as_u8(255.0 * _g(m + e, gamma) + BAND_ARG_SLACK)


def _arg_lo(c, gamma):
    """The low end of the widened argument: no slack where min(c, 1) is 1 (both sides then compute 255 exactly)."""
    return np.where(np.asarray(c) >= 1.0, 255.0, 255.0 * _g(c, gamma) - BAND_ARG_SLACK)


def band_check(got_u8, ref_u8, mean, max_abs, gamma=False, eps_rel=BAND_EPS_REL, eps_abs=BAND_EPS_ABS):
    """Judges device bytes `got_u8` against the oracle's float64 means (band_stats), never wider than the ceiling."""
    assert eps_rel <= BAND_EPS_REL_MAX and eps_abs <= BAND_EPS_ABS_MAX, "band wider than the ceiling (DESIGN.md section 4)"
    return band_stats(got_u8, ref_u8, mean, max_abs, gamma, eps_rel, eps_abs)


def band_stats(got_u8, ref_u8, mean, max_abs, gamma=False, eps_rel=BAND_EPS_REL, eps_abs=BAND_EPS_ABS):
    """Judges bytes `got_u8` against float64 means.  Non-finite means (D6 flags) must give the oracle's own byte
    `ref_u8`; channels whose largest sample component exceeds D6_CLAMP are excluded and counted.  Returns counts, the
    worst miss (LSB, on the argument of as_u8) and band_eps_scale: the smallest factor on (eps_rel, eps_abs) with which
    every judged channel would still pass (0 if each byte is q(m) itself)."""
    b = np.asarray(got_u8).astype(np.int32)
    m = np.asarray(mean, np.float64)
    gamma = np.broadcast_to(np.asarray(gamma, bool), m.shape)
    finite = np.isfinite(m)
    d6 = finite & (np.asarray(max_abs, np.float64) > D6_CLAMP)
    judged = finite & ~d6
    nf_diff = ~finite & (b != np.asarray(ref_u8).astype(np.int32))
    mj, bj, gj = np.where(judged, m, 0.0), b, gamma
    e = eps_rel * np.abs(mj) + eps_abs
    x_lo = _arg_lo(mj - e, gj)
    x_hi = 255.0 * _g(mj + e, gj) + BAND_ARG_SLACK
    lo, hi = as_u8(x_lo), as_u8(x_hi)
    outside = judged & ((bj < lo) | (bj > hi))
    miss = np.where(bj > hi, bj - x_hi, np.where(bj < lo, x_lo - (bj + 1), 0.0))
    # the e each channel needs: the edge of its byte's preimage, seen from m (with the argument slack kept)
    lo0, hi0 = band_bytes(mj, gj, 0.0, 0.0)
    need_up = _g_inv((bj - BAND_ARG_SLACK) / 255.0, gj) - mj
    need_dn = mj - _g_inv((bj + 1 + BAND_ARG_SLACK) / 255.0, gj)
    need = np.where(bj > hi0, need_up, np.where(bj < lo0, need_dn, 0.0))
    scale = np.where(judged, np.maximum(need, 0.0) / (eps_rel * np.abs(mj) + eps_abs), 0.0)
    return dict(n_rgb_checked=int(judged.sum()), n_rgb_in_band=int((judged & (hi > lo)).sum()),
                n_rgb_outside_band=int(outside.sum() + nf_diff.sum()),
                n_rgb_nonfinite=int((~finite).sum()), n_rgb_d6_excluded=int(d6.sum()),
                band_worst_miss_lsb=float(np.where(outside, miss, 0.0).max()) if b.size else 0.0,
                band_eps_scale=float(scale.max()) if b.size else 0.0)


def depth_check(got, ref, mean, abs_err=DEPTH_HALF_STEP, rel_err=4 * U32):
    """|got - m| <= 2^-17 + 4u|m| (half a 2^-16 accumulator step, the double -> float and /n roundings).  A non-finite
    mean must give the oracle's own value (NaN for NaN, whatever its sign and payload)."""
    g, r, m = (np.asarray(x) for x in (got, ref, mean))
    finite = np.isfinite(m)
    bound = abs_err + rel_err * np.abs(np.where(finite, m, 0.0))
    err = np.abs(g.astype(np.float64) - np.where(finite, m, 0.0))
    bad = finite & ~(err <= bound)
    bad |= ~finite & ~((np.isnan(g) & np.isnan(r)) | (g == r))
    return dict(n_depth_outside=int(bad.sum()),
                depth_scale=float(np.where(finite & (bound > 0), err / np.where(bound > 0, bound, 1.0), 0.0).max()) if g.size else 0.0)


def normal_check(got, mean, term_err=NORMAL_TERM_ERR):
    """The device normal against normalize(m): each component within 2*sqrt(3)*2^-25/|m| (a per-component error of
    2^-25 turns the unit vector by at most twice its length over |m|) plus 8u for the f32 sum, /n and normalise.
    Pixels with |m| < 1e-3 or a non-finite mean are skipped and counted (their NaN pattern is compared elsewhere)."""
    g = np.asarray(got, np.float64)
    m = np.asarray(mean, np.float64)
    with np.errstate(invalid="ignore"):
        nrm = np.sqrt((m * m).sum(axis=-1))
    ok = np.isfinite(nrm) & (nrm >= NORMAL_MIN_NORM)
    unit = m / np.where(ok, nrm, 1.0)[..., None]
    bound = 2 * np.sqrt(3.0) * term_err / np.where(ok, nrm, 1.0) + 8 * U32
    with np.errstate(invalid="ignore"):
        err = np.abs(g - unit).max(axis=-1)
    bad = ok & ~(err <= bound)
    return dict(n_normal_outside=int(bad.sum()), n_normal_skipped=int((~ok).sum()),
                normal_scale=float(np.where(ok, err / bound, 0.0).max()) if ok.size else 0.0)


def compare_frames(a: dict, b: dict, rgb_tol: int = 1, eps_rel: float = BAND_EPS_REL, eps_abs: float = BAND_EPS_ABS):
    """Returns a dict of mismatch statistics between two renders (a = candidate, b = oracle).  When `b` carries the
    oracle's float64 means (render(..., want_means=True)) the band, depth and normal statistics are added
    (band_check, depth_check, normal_check)."""
    ra, rb = a["rgba"].astype(np.int32), b["rgba"].astype(np.int32)
    diff = np.abs(ra[..., :3] - rb[..., :3]).max(axis=-1)
    res = dict(max_rgb_diff=int(diff.max()), n_rgb_over=int((diff > rgb_tol).sum()), n_pixels=int(diff.size),
               alpha_ok=bool((ra[..., 3] == 255).all()))
    if "object_id" in a and "object_id" in b:
        res["n_id_diff"] = int((a["object_id"] != b["object_id"]).sum())
    if "depth" in a and "depth" in b:
        da, db = a["depth"].astype(np.float64), b["depth"].astype(np.float64)
        res["max_depth_rel"] = float((np.abs(da - db) / np.maximum(np.abs(db), 1e-3)).max())
    if "normal" in a and "normal" in b:
        na, nb = a["normal"], b["normal"]
        both_nan = np.isnan(na) & np.isnan(nb)
        d = np.where(both_nan, 0.0, np.abs(na.astype(np.float64) - nb.astype(np.float64)))
        res["nan_mismatch"] = int((np.isnan(na) != np.isnan(nb)).sum())
        res["max_normal_abs"] = float(np.nanmax(d)) if d.size else 0.0
    if "mean_rgb" in b:
        res.update(band_check(a["rgba"][..., :3], b["rgba"][..., :3], b["mean_rgb"], b["max_abs_rgb"],
                              b["mean_gamma"][..., None], eps_rel, eps_abs))
        if "depth" in a:
            res.update(depth_check(a["depth"], b["depth"], b["mean_depth"]))
        if "normal" in a:
            res.update(normal_check(a["normal"], b["mean_normal"]))
        _log_band(res)
    return res


def assert_in_band(res: dict, what: str = ""):
    """The float64-mean checks of compare_frames all hold (requires a reference rendered with want_means=True)."""
    assert "n_rgb_outside_band" in res, f"{what}: the reference carries no means"
    assert res["n_rgb_outside_band"] == 0, f"{what}: {res}"
    assert res.get("n_depth_outside", 0) == 0 and res.get("n_normal_outside", 0) == 0, f"{what}: {res}"


def _log_band(res: dict):
    """RR_BAND_LOG=<file>: one JSON line per comparison with means (test id and margins), for reviewing the bar."""
    path = os.environ.get("RR_BAND_LOG")
    if not path:
        return
    import json
    keys = ("n_rgb_checked", "n_rgb_in_band", "n_rgb_outside_band", "n_rgb_d6_excluded", "n_rgb_nonfinite",
            "band_worst_miss_lsb", "band_eps_scale", "n_depth_outside", "depth_scale", "n_normal_outside",
            "n_normal_skipped", "normal_scale", "max_rgb_diff")
    rec = {"test": os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0], **{k: res[k] for k in keys if k in res}}
    with open(path, "a") as f:
        f.write(json.dumps(rec) + "\n")


def assert_frames_identical(a: dict, b: dict, what: str = ""):
    """rgba, depth, normal and object_id equal bit for bit (floats compared as their bit patterns, NaN payloads included)."""
    for k in ("rgba", "depth", "normal", "object_id"):
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.dtype == np.float32:
            x, y = x.view(np.uint32), y.view(np.uint32)
        assert x.shape == y.shape and np.array_equal(x, y), f"{what}: {k} differs in {int((x != y).sum())} values"


def item_transforms(fs: FlatScene, dx: float = 0.0):
    """(n, 4, 4) float32 transforms and inverses of the scene's items (math layout), every item moved by (dx, 0, 0)."""
    t = np.stack([np.asarray(it.trans, np.float64) for it in fs.items]) if fs.items else np.zeros((0, 4, 4))
    ti = np.stack([np.asarray(it.trans_inv, np.float64) for it in fs.items]) if fs.items else np.zeros((0, 4, 4))
    move, back = np.eye(4), np.eye(4)
    move[0, 3], back[0, 3] = dx, -dx
    return (move @ t).astype(np.float32), (ti @ back).astype(np.float32)


def with_transforms(fs: FlatScene, t, ti) -> FlatScene:
    """A copy of the scene whose items carry the given transforms (what a freshly created scene is built from)."""
    import copy
    out = copy.deepcopy(fs)
    for it, a, b in zip(out.items, t, ti):
        it.trans, it.trans_inv = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return out
