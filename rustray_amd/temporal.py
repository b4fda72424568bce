"""The temporal reprojection of rr_accumulate_records in numpy float32: the yardstick the device kernel and the host loop over
rustray_amd/csrc/rr_temporal.h are held to, bit for bit.

Every step is exact in binary32 in the order include/rustray_hip.h states: float32 products and sums one at a time (numpy does not
contract), one correctly rounded division or square root at a time, no transcendentals.  The up to four taps of a pixel are four
whole-frame gathers here; a tap that is skipped adds nothing (np.add(..., where=taken)), so the sums are those of the per-pixel loop.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from .pixel_rays import camera_matrices, dot, pixel_rays, row

F = np.float32
EPS = F(2.0 ** -20)
MIN_WEIGHT = F(2.0 ** -6)


@dataclass
class HistoryClampParams:
    """rr_history_clamp_params without its struct_size; the defaults are rr_history_clamp_default_params'."""
    radius: int = 1
    sigma_scale: float = 0.5

    def check(self):
        if self.radius not in (1, 2):
            raise ValueError(f"radius {self.radius} (1 or 2)")
        k = F(self.sigma_scale)
        if not (np.isfinite(k) and 0.0 <= float(k) <= 65536.0):
            raise ValueError(f"sigma_scale {self.sigma_scale} (finite, 0 .. 65536)")


@dataclass
class AccumulateParams:
    """rr_accumulate_params without its struct_size; the defaults are rr_accumulate_default_params'.  prev_world_to_clip is the 4x4
    matrix as written on paper (row r, column c), the C struct holds it column-major."""
    prev_world_to_clip: np.ndarray = field(default_factory=lambda: np.eye(4, dtype=F))
    prev_eye: np.ndarray = field(default_factory=lambda: np.zeros(3, F))
    max_history: float = 32.0
    normal_min: float = 0.9
    sigma_depth: float = 0.05
    snap: float = 1.0 / 64.0
    gamma_correction: bool = False

    def check(self):
        if np.asarray(self.prev_world_to_clip).shape != (4, 4) or np.asarray(self.prev_eye).shape != (3,):
            raise ValueError("prev_world_to_clip is 4x4, prev_eye has 3 floats")
        if not 1.0 <= float(F(self.max_history)) <= 65536.0:
            raise ValueError(f"max_history {self.max_history} (1 .. 65536)")
        if not -1.0 <= float(F(self.normal_min)) <= 1.0:
            raise ValueError(f"normal_min {self.normal_min} (-1 .. 1)")
        if not (float(F(self.sigma_depth)) > 0.0 and np.isfinite(F(self.sigma_depth))):
            raise ValueError("sigma_depth must be finite and above 0")
        if not 0.0 <= float(F(self.snap)) < 0.5:
            raise ValueError(f"snap {self.snap} (0 <= snap < 0.5)")


def previous_view(camera):
    """(world_to_clip (4, 4) float32, eye (3,) float32) of a camera.Camera: what the NEXT frame's AccumulateParams take as
    prev_world_to_clip and prev_eye.  The product is formed in float64 and rounded once.  An rr_camera, which holds only the
    inverses, is inverted in float64."""
    if hasattr(camera, "projection"):
        m = np.asarray(camera.projection, np.float64) @ np.asarray(camera.view, np.float64)
        return m.astype(F), np.asarray(camera.view_inverse, np.float64)[:3, 3].astype(F)
    pi = np.array(camera.projection_inverse[:], np.float64).reshape(4, 4).T
    vi = np.array(camera.view_inverse[:], np.float64).reshape(4, 4).T
    return (np.linalg.inv(pi) @ np.linalg.inv(vi)).astype(F), vi[:3, 3].astype(F)


def world_positions(records, cam) -> np.ndarray:
    """(n, 3) float32: world_p = o + d * depth_p of every record of a whole frame of `cam`, o and d the pinhole ray through the pixel's
    centre, in the header's arithmetic (step 2)."""
    _, _, W, H = camera_matrices(cam)
    rec = np.ascontiguousarray(records, F).reshape(H * W, 8)
    o, d = pixel_rays(cam)
    with np.errstate(all="ignore"):
        return (o + d * rec[:, 3:4]).astype(F)


def item_motion(world, object_id, item_ids, prev_trans, cur_trans_inv) -> np.ndarray:
    """The `motion` of rigidly moving items: for every pixel whose object id is item_ids[i], prev_trans[i] @ cur_trans_inv[i] @ world_p
    - world_p (the point in the item's own space, placed where the item stood one rr_scene_update_transforms step ago); 0 elsewhere.
    world (n, 3), object_id (n,), item_ids (k,), prev_trans and cur_trans_inv (k, 4, 4) as written on paper.  float64 inside, rounded once."""
    world = np.asarray(world, np.float64)
    ids = np.asarray(object_id).astype(np.int64)
    out = np.zeros((len(world), 3), F)
    for ident, a, b in zip(np.asarray(item_ids).astype(np.int64), np.asarray(prev_trans, np.float64), np.asarray(cur_trans_inv, np.float64)):
        at = np.flatnonzero((ids == ident) & np.isfinite(world).all(-1))
        if len(at):
            p = np.concatenate([world[at], np.ones((len(at), 1))], axis=1) @ (a @ b).T
            out[at] = (p[:, :3] - world[at]).astype(F)
    return out


def motion_records(records, cam, item_ids, prev_trans, cur_trans_inv):
    """rr_motion_records in numpy float32, the yardstick the kernel k_motion_records and the host loop over rustray_amd/csrc/rr_motion.h
    equal bit for bit: records (n, 8) of the whole frame of `cam`; item_ids (k,) the object ids of the moved items (no two alike),
    prev_trans (k, 4, 4) their `trans` in the frame of the history and cur_trans_inv (k, 4, 4) their `trans_inv` in the current one,
    as written on paper.  -> (motion (n, 3), world (n, 3)): world is world_positions(records, cam); motion is 0 unless the record is
    valid (depth and normal finite) and its object id is listed, and then row(prev_trans, r, (row(trans_inv, ., (world, 1)), 1)) -
    world_r, all three 0 if one of them is not finite."""
    world = world_positions(records, cam)
    n = len(world)
    rec = np.ascontiguousarray(records, F).reshape(n, 8)
    ids = np.asarray(item_ids).astype(np.uint32).reshape(-1)
    if len(np.unique(ids)) != len(ids):
        raise ValueError("two moved items have the same object id")
    prev = np.asarray(prev_trans, F).reshape(len(ids), 4, 4)
    inv = np.asarray(cur_trans_inv, F).reshape(len(ids), 4, 4)
    valid = np.isfinite(rec[:, 3]) & np.isfinite(rec[:, 4:7]).all(-1)
    ids_p = rec[:, 7].view(np.uint32)
    motion = np.zeros((n, 3), F)
    one = F(1)
    with np.errstate(all="ignore"):
        for ident, a, b in zip(ids, prev, inv):
            at = np.flatnonzero(valid & (ids_p == ident))
            if not len(at):
                continue
            w = world[at]
            a_cm, b_cm = a.T.reshape(16), b.T.reshape(16)      # column-major, as the C arrays
            local = [row(b_cm, r, w[:, 0], w[:, 1], w[:, 2], one) for r in range(3)]
            m = np.stack([row(a_cm, r, local[0], local[1], local[2], one) - w[:, r] for r in range(3)], axis=-1).astype(F)
            m[~np.isfinite(m).all(-1)] = F(0)
            motion[at] = m
    return motion, world


def _accumulate(records, halves, history, history_halves, history_length, motion, cam, prm, extra=(), hook=None):
    """The tap walk and the blends that accumulate_records, accumulate_split_records and accumulate_clamped_records share.  extra: (current
    (n, 3), history (n, 3) or None) per extra layer, which rides on the taps and weights of the records and decides nothing.  hook (or
    None): called between the means and the blend as hook(rec, means, N, kept, means_x) with the history means of the records and the two
    halves (a list of (n, 3)) and those of the extra layers (another), and gives (means, N, means_x) back -- what accumulate_clamped_records
    and accumulate_clamped_split_records do to them.  An extra layer is blended where its current triple and the mean the hook gave back are
    finite.  -> (accumulate_records' dict, the extra layers' outputs)."""
    prm.check()
    pi, vi, W, H = camera_matrices(cam)
    n = W * H
    rec = np.ascontiguousarray(records, F).reshape(n, 8)
    hv = None if halves is None else np.ascontiguousarray(halves, F).reshape(n, 2, 8)
    if (history is None) != (history_length is None):
        raise ValueError("history and history_length come together")
    if history is not None and (history_halves is None) != (hv is None) or history is None and history_halves is not None:
        raise ValueError("history_halves is required exactly when history and halves are given")
    m = np.asarray(prm.prev_world_to_clip, F).T.reshape(16)   # column-major, as the C struct
    eye = np.asarray(prm.prev_eye, F)
    max_history, normal_min, sigma_depth, snap = F(prm.max_history), F(prm.normal_min), F(prm.sigma_depth), F(prm.snap)
    one, half = F(1), F(0.5)

    out = rec.copy()
    out_h = None if hv is None else hv.copy()
    out_x = [np.array(cur, F).reshape(n, 3) for cur, _ in extra]
    taps = dict(x=np.zeros((n, 4), np.int64), y=np.zeros((n, 4), np.int64), weight=np.zeros((n, 4), F), taken=np.zeros((n, 4), bool),
                reprojected=np.zeros(n, bool))
    with np.errstate(all="ignore"):
        fin = np.isfinite(rec[:, 0:3]).all(-1)
        valid = np.isfinite(rec[:, 3]) & np.isfinite(rec[:, 4:7]).all(-1)
        length = np.where(fin, one, F(0)).astype(F)
        if history is None:
            return dict(records=out, length=length, halves=out_h, taps=taps), out_x
        hist = np.ascontiguousarray(history, F).reshape(n, 8)
        hist_h = None if hv is None else np.ascontiguousarray(history_halves, F).reshape(n, 2, 8)
        hist_len = np.ascontiguousarray(history_length, F).reshape(n)
        hist_x = [np.ascontiguousarray(h, F).reshape(n, 3) for _, h in extra]
        sum_x = [np.zeros((n, 3), F) for _ in extra]
        prev = world_positions(rec, cam)
        if motion is not None:
            prev = prev + np.ascontiguousarray(motion, F).reshape(n, 3)
        px, py, pz = prev[:, 0], prev[:, 1], prev[:, 2]
        cx, cy, cw = row(m, 0, px, py, pz, one), row(m, 1, px, py, pz, one), row(m, 3, px, py, pz, one)
        alive = fin & valid & (cw > EPS)
        fx = ((cx / cw) * half + half) * F(W) - half
        fy = (half - (cy / cw) * half) * F(H) - half
        alive &= np.isfinite(fx) & np.isfinite(fy)
        alive &= (fx > F(-1)) & (fx < F(W)) & (fy > F(-1)) & (fy < F(H))
        e = prev - eye
        dist = np.sqrt(dot(e, e))
        z_exp = dist - dist / cw

        fx, fy = np.where(alive, fx, F(0)), np.where(alive, fy, F(0))   # (so that the integer conversions below are defined)
        rx, ry = np.rint(fx), np.rint(fy)
        snapped = (np.abs(fx - rx) <= snap) & (np.abs(fy - ry) <= snap)
        x0f, y0f = np.floor(fx), np.floor(fy)
        tx, ty = np.where(snapped, F(0), fx - x0f), np.where(snapped, F(0), fy - y0f)
        x0 = np.where(snapped, rx, x0f).astype(np.int64)
        y0 = np.where(snapped, ry, y0f).astype(np.int64)
        n_taps = np.where(snapped, 1, 4)

        ids_p, n_p = rec[:, 7].view(np.uint32), rec[:, 4:7]
        layers = [hist[:, 0:3]] + ([] if hv is None else [hist_h[:, 0, 0:3], hist_h[:, 1, 0:3]])
        sum_c = [np.zeros((n, 3), F) for _ in layers]
        sum_w, sum_l = np.zeros(n, F), np.zeros(n, F)
        for k in range(4):
            qx, qy = x0 + (k & 1), y0 + (k >> 1)
            inside = (qx >= 0) & (qy >= 0) & (qx < W) & (qy < H)
            q = np.where(inside, qy * W + qx, 0)
            taken = alive & (k < n_taps) & inside
            n_q = hist[q, 4:7]
            taken &= (hist[q, 7].view(np.uint32) == ids_p) & np.isfinite(n_q).all(-1) & (dot(n_p, n_q) >= normal_min)
            taken &= np.isfinite(hist[q, 0:3]).all(-1) & np.isfinite(hist[q, 3]) & (np.abs(z_exp - hist[q, 3]) <= sigma_depth * z_exp + EPS)
            taken &= hist_len[q] > 0
            if hv is not None:
                taken &= np.isfinite(hist_h[q, 0, 0:3]).all(-1) & np.isfinite(hist_h[q, 1, 0:3]).all(-1)
            w = ((tx if k & 1 else one - tx) * (ty if k >> 1 else one - ty)).astype(F)
            for s, layer in zip(sum_c, layers):
                np.add(s, w[:, None] * layer[q], out=s, where=taken[:, None])
            for sx, layer in zip(sum_x, hist_x):
                np.add(sx, w[:, None] * layer[q], out=sx, where=taken[:, None])
            np.add(sum_l, w * hist_len[q], out=sum_l, where=taken)
            np.add(sum_w, w, out=sum_w, where=taken)
            taps["x"][:, k], taps["y"][:, k], taps["weight"][:, k], taps["taken"][:, k] = qx, qy, w, taken
        kept = alive & (sum_w >= MIN_WEIGHT)
        taps["taken"] &= kept[:, None]
        taps["reprojected"] = alive
        n1 = sum_l / sum_w + one
        N = np.where(n1 < max_history, n1, max_history).astype(F)
        means = [s / sum_w[:, None] for s in sum_c]
        means_x = [sx / sum_w[:, None] for sx in sum_x]
        if hook is not None:
            means, N, means_x = hook(rec, means, N, kept, means_x)
        a = one / N
        currents = [rec[:, 0:3]] + ([] if hv is None else [hv[:, 0, 0:3], hv[:, 1, 0:3]])
        targets = [out[:, 0:3]] + ([] if hv is None else [out_h[:, 0, 0:3], out_h[:, 1, 0:3]])
        for h, cur, dst in zip(means, currents, targets):
            blended = h + a[:, None] * (cur - h)
            dst[...] = np.where((kept & np.isfinite(cur).all(-1))[:, None], blended, cur)
        for hd, (cur, _), dst in zip(means_x, extra, out_x):
            cur = np.ascontiguousarray(cur, F).reshape(n, 3)
            blended = hd + a[:, None] * (cur - hd)
            dst[...] = np.where((kept & np.isfinite(cur).all(-1) & np.isfinite(hd).all(-1))[:, None], blended, cur)
        length = np.where(kept, N, length).astype(F)
    return dict(records=out, length=length, halves=out_h, taps=taps), out_x


def accumulate_records(records, halves, history, history_halves, history_length, motion, cam, params: AccumulateParams | None = None) -> dict:
    """records (n, 8) float32 rr_radiance records of the whole frame of `cam` (a camera.Camera or an rr_camera) in row-major order;
    halves (n, 2, 8) or None; history (n, 8), history_halves (n, 2, 8) and history_length (n,): the previous call's records, halves and
    length, or all None on the first frame; motion (n, 3) or None.  Returns dict(records (n, 8), length (n,), halves (n, 2, 8) or None,
    taps: dict(x, y (n, 4) int, weight (n, 4) float32, taken (n, 4) bool, reprojected (n,) bool: the pixel reached step 4) -- where each
    pixel's history came from)."""
    return _accumulate(records, halves, history, history_halves, history_length, motion, cam, params or AccumulateParams())[0]


def accumulate_split_records(records, halves, diffuse, diffuse_halves, history, history_halves, history_diffuse, history_diffuse_halves, history_length,
                             motion, cam, params: AccumulateParams | None = None, _hook=None) -> dict:
    """rr_accumulate_split_records in numpy float32: accumulate_records' arguments, and diffuse (n, 3), diffuse_halves (n, 2, 3) or None
    (exactly when halves is), history_diffuse (n, 3) exactly when history is given and history_diffuse_halves (n, 2, 3) exactly when
    history_halves is.  The diffuse layers ride on the taps, weights and length of the records: records, halves and length are
    accumulate_records' bits.  A diffuse layer of a kept pixel is hd + a * (cur - hd) where its current triple and its history mean hd are
    finite, and its current bits everywhere else.  -> dict(records (n, 8), halves (n, 2, 8) or None, diffuse (n, 3), diffuse_halves
    (n, 2, 3) or None, length (n,), taps)."""
    if diffuse is None:
        raise ValueError("diffuse is required")
    if (diffuse_halves is None) != (halves is None):
        raise ValueError("diffuse_halves is required exactly when halves is given")
    if (history_diffuse is None) != (history is None):
        raise ValueError("history_diffuse is required exactly when history is given")
    if (history_diffuse_halves is None) != (history_halves is None):
        raise ValueError("history_diffuse_halves is required exactly when history_halves is given")
    n = np.ascontiguousarray(records, F).size // 8
    layer = lambda a, h: None if a is None else np.ascontiguousarray(a, F).reshape(n, 2, 3)[:, h]
    flat = lambda a: None if a is None else np.ascontiguousarray(a, F).reshape(n, 3)
    extra = [(flat(diffuse), flat(history_diffuse))]
    if diffuse_halves is not None:
        extra += [(layer(diffuse_halves, h), layer(history_diffuse_halves, h)) for h in (0, 1)]
    res, out_x = _accumulate(records, halves, history, history_halves, history_length, motion, cam, params or AccumulateParams(), extra, _hook)
    res["diffuse"] = out_x[0]
    res["diffuse_halves"] = None if diffuse_halves is None else np.ascontiguousarray(np.stack([out_x[1], out_x[2]], axis=1))
    return res


def clamp_boxes(records, W: int, H: int, clamp: HistoryClampParams):
    """Step 7 of rr_accumulate_clamped_records for every pixel of a W x H frame of records (n, 8): (lo, hi, e), each (n, 3) float32, and m
    (n,), how many pixels of the window were taken.  The (2r + 1)^2 window positions are whole-frame shifts here, in the header's order; a
    position that is not taken adds nothing.  A channel without a box has lo = -inf, hi = e = +inf.  (A pixel whose own colour is not
    finite never reaches step 7; what stands here for it means nothing.)  `records` may also be an (n, 3) array of triples, the current
    `diffuse` layer of rr_accumulate_clamped_split_records: a position is taken on its three floats in the same way, the pixel itself
    included, and a window in which nothing is taken has m = 0, a NaN mean and no box."""
    r, k = int(clamp.radius), F(clamp.sigma_scale)
    col = np.ascontiguousarray(records, F).reshape(H, W, -1)[:, :, 0:3]
    ok = np.isfinite(col).all(-1)
    m = np.zeros((H, W), np.int64)
    s1, s2 = np.zeros((H, W, 3), F), np.zeros((H, W, 3), F)
    with np.errstate(all="ignore"):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                ys, yq = slice(max(0, -dy), min(H, H - dy)), slice(max(0, dy), min(H, H + dy))
                xs, xq = slice(max(0, -dx), min(W, W - dx)), slice(max(0, dx), min(W, W + dx))
                if ys.start >= ys.stop or xs.start >= xs.stop:
                    continue
                t, c = ok[yq, xq], col[yq, xq]
                m[ys, xs] += t
                np.add(s1[ys, xs], c, out=s1[ys, xs], where=t[..., None])
                np.add(s2[ys, xs], c * c, out=s2[ys, xs], where=t[..., None])
        mf = m.astype(F)[..., None]
        mean = s1 / mf
        q, mm = s2 / mf, mean * mean
        v = q - mm
        sd = np.sqrt(np.where(v > 0, v, F(0)).astype(F))
        e = (k * sd).astype(F)
        boxed = np.isfinite(q) & np.isfinite(mm) & np.isfinite(e)
        lo = np.where(boxed, mean - e, F(-np.inf)).astype(F).reshape(-1, 3)
        hi = np.where(boxed, mean + e, F(np.inf)).astype(F).reshape(-1, 3)
        e = np.where(boxed, e, F(np.inf)).astype(F).reshape(-1, 3)
    return lo, hi, e, m.reshape(-1)


def _colour_clamp_hook(lo, hi, e, clamped):
    """Steps 8 and 9 of rr_accumulate_clamped_records as _accumulate's hook: the means of the records and the halves held to the box (lo, hi,
    e: clamp_boxes'), the length shortened where the record layer was moved; `clamped` (n, 3) bool is filled per layer.  The extra layers'
    means pass through."""
    one = F(1)

    def hook(rec, means, N, kept, means_x):
        held, moved = [], []
        for h in means:
            below, above = h < lo, h > hi
            held.append(np.where(below, lo, np.where(above, hi, h)).astype(F))
            moved.append((below | above) & kept[:, None])
        for layer, mv in enumerate(moved):
            clamped[:, layer] = mv.any(-1)
        u = np.where(moved[0], np.abs(means[0] - held[0]) / (e + EPS), F(0)).astype(F)
        t01 = np.where(u[:, 0] > u[:, 1], u[:, 0], u[:, 1])
        t = np.where(t01 > u[:, 2], t01, u[:, 2])
        keep = one / (one + t)
        shorter = ((N - one) * keep + one).astype(F)
        return held, np.where(clamped[:, 0], shorter, N).astype(F), means_x

    return hook


def accumulate_clamped_records(records, halves, history, history_halves, history_length, motion, cam, params: AccumulateParams | None = None,
                               clamp: HistoryClampParams | None = None) -> dict:
    """rr_accumulate_clamped_records in numpy float32, following steps 7 .. 10 of its text in include/rustray_hip.h: accumulate_records'
    arguments and a HistoryClampParams (None: the defaults).  The history means of a kept pixel are held to the box of the current
    frame's colours around it, and the length is shortened where the record layer had to be moved.  -> accumulate_records' dict, and
    clamped (n, 3) bool: per layer (records, half 0, half 1) whether a channel of that layer's mean was moved (False for a pixel
    without history and for a layer the call does not have), and box: dict(lo (n, 3), hi (n, 3))."""
    clamp = clamp or HistoryClampParams()
    clamp.check()
    _, _, W, H = camera_matrices(cam)
    lo, hi, e, _ = clamp_boxes(records, W, H, clamp)
    clamped = np.zeros((W * H, 3), bool)
    res = _accumulate(records, halves, history, history_halves, history_length, motion, cam, params or AccumulateParams(),
                      hook=_colour_clamp_hook(lo, hi, e, clamped))[0]
    res["clamped"] = clamped
    res["box"] = dict(lo=lo, hi=hi)
    return res


def accumulate_clamped_split_records(records, halves, diffuse, diffuse_halves, history, history_halves, history_diffuse, history_diffuse_halves,
                                     history_length, motion, cam, params: AccumulateParams | None = None, clamp: HistoryClampParams | None = None) -> dict:
    """rr_accumulate_clamped_split_records in numpy float32, following its text in include/rustray_hip.h: accumulate_split_records'
    arguments and a HistoryClampParams (None: the defaults).  The colour side is accumulate_clamped_records' (records, halves and length are
    its bits); each diffuse mean of a kept pixel is held to the box of the current `diffuse` layer around it where that mean and the
    layer's current triple are finite, and blended with the colour side's final a.  -> accumulate_split_records' dict, and clamped (n, 3)
    bool as accumulate_clamped_records gives it, diffuse_clamped (n, 3) bool: per diffuse layer (diffuse, half 0, half 1) whether a channel
    of its mean was moved in a blend that took place (False for a pixel without history, a layer that keeps its current bits and a layer
    the call does not have), box: dict(lo, hi) of the colours and diffuse_box: dict(lo, hi) of the diffuse layer, each (n, 3)."""
    clamp = clamp or HistoryClampParams()
    clamp.check()
    if diffuse is None:
        raise ValueError("diffuse is required")
    _, _, W, H = camera_matrices(cam)
    n = W * H
    lo, hi, e, _ = clamp_boxes(records, W, H, clamp)
    cur_d = np.ascontiguousarray(diffuse, F).reshape(n, 3)
    dlo, dhi, _, _ = clamp_boxes(cur_d, W, H, clamp)
    clamped, diffuse_clamped = np.zeros((n, 3), bool), np.zeros((n, 3), bool)
    colour_hook = _colour_clamp_hook(lo, hi, e, clamped)
    currents = [cur_d] + ([] if diffuse_halves is None else [np.ascontiguousarray(diffuse_halves, F).reshape(n, 2, 3)[:, h] for h in (0, 1)])

    def hook(rec, means, N, kept, means_x):
        held, N, _ = colour_hook(rec, means, N, kept, means_x)
        held_x = []
        for layer, (hd, cur) in enumerate(zip(means_x, currents)):
            blends = kept & np.isfinite(cur).all(-1) & np.isfinite(hd).all(-1)
            below, above = (hd < dlo) & blends[:, None], (hd > dhi) & blends[:, None]
            held_x.append(np.where(below, dlo, np.where(above, dhi, hd)).astype(F))
            diffuse_clamped[:, layer] = (below | above).any(-1)
        return held, N, held_x

    res = accumulate_split_records(records, halves, diffuse, diffuse_halves, history, history_halves, history_diffuse, history_diffuse_halves, history_length,
                                   motion, cam, params, _hook=hook)
    res["clamped"], res["diffuse_clamped"] = clamped, diffuse_clamped
    res["box"], res["diffuse_box"] = dict(lo=lo, hi=hi), dict(lo=dlo, hi=dhi)
    return res
