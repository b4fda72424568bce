"""Where a surface point seen by one camera lay in the frame of another, in float64, from the cameras' definition: the truth the temporal
reprojection (rr_accumulate_records and its split and clamped forms, rustray_amd/temporal.py, rustray_amd/csrc/rr_temporal.h) is held to
by tests/test_reprojection_host.py and tests/test_gpu_reprojection.py.  numpy only, no GPU.

The kernel, the host loop and the float32 yardstick were written from one reading of include/rustray_hip.h, so the suite's bit-for-bit
comparisons cannot see what the three share: the pixel-centre convention and the y flip, the ray origin on the plane one unit ahead of
the eye (z_exp = dist - dist / clip.w), which tap bit is x, the order of prev_world_to_clip, which camera is the "previous" one.
Nothing here reads Camera.projection, .view, temporal.previous_view or pixel_rays: a camera is its eye, an orthonormal basis made from
dir and up, tan(fov / 2) and the aspect ratio, and a pixel is a square of the image plane.

Frames of ONE sample without depth of field only: a record's depth is then the centre ray's.  With more samples the mean depth is not
the depth along the centre ray, the reprojected position is off by a property of the design (not a bug), and these bounds do not apply.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import numpy as np

from rustray_amd.camera import Camera

F = np.float32
EPS = 2.0 ** -20           # the header's EPS
MIN_WEIGHT = 2.0 ** -6     # "no history unless sum_w >= 2^-6"
POS_TOL = 2.0 ** -14       # pixels: the position bound, and how close to a cell or snap boundary counts as borderline
REL_TOL = 1e-4             # how close to a threshold (relative) counts as borderline
OUTSIDE_TOL = 2.0 ** -10   # pixels: a true position this far outside (-1, W) x (-1, H) must have no history
SIZES = ((64, 48), (37, 29))


@dataclass(frozen=True)
class Pinhole:
    eye: np.ndarray       # (3,)
    right: np.ndarray     # unit, x of the image grows along it
    up: np.ndarray        # unit, y of the image DECREASES along it (row 0 is the top row)
    ahead: np.ndarray     # unit, the viewing direction
    tan_half: float       # tan(fov / 2): half the image plane's height at distance 1
    aspect: float         # width / height of the image plane


def _unit(v):
    return v / math.sqrt(float(v @ v))


def pinhole(camera) -> Pinhole:
    """The camera of a camera.Camera from its definition: eye, dir, up, fov (vertical) and aspect ratio, each rounded to float32 first
    as the fields of the reference's camera are, everything after that in float64.  Right-handed: right = ahead x up."""
    f32 = lambda v: np.asarray(v, F).astype(np.float64)
    ahead = _unit(f32(camera.dir))
    right = _unit(np.cross(ahead, f32(camera.up)))
    return Pinhole(eye=f32(camera.eye_pos), right=right, up=np.cross(right, ahead), ahead=ahead,
                   tan_half=math.tan(float(F(camera.fov)) / 2.0), aspect=float(F(camera.aspect_ratio)))


def forward(pin: Pinhole, fx, fy, W: int, H: int):
    """The ray through the continuous pixel position (fx, fy) of a W x H frame; integer positions are pixel centres, (-0.5, -0.5) is the
    frame's top left corner.  -> (origin (..., 3) on the plane one unit ahead of the eye, unit direction (..., 3))."""
    fx, fy = np.asarray(fx, np.float64), np.asarray(fy, np.float64)
    sx = ((fx + 0.5) / W * 2.0 - 1.0) * pin.tan_half * pin.aspect
    sy = (1.0 - (fy + 0.5) / H * 2.0) * pin.tan_half
    off = pin.ahead + sx[..., None] * pin.right + sy[..., None] * pin.up
    return pin.eye + off, off / np.sqrt((off * off).sum(-1))[..., None]


def inverse(pin: Pinhole, P, W: int, H: int):
    """Where the world points P (..., 3) lie in the W x H frame of `pin` -> (fx, fy, zc, z_exp): the continuous pixel position, the
    distance ahead of the eye, and the depth a record of that frame holds for the point, measured along the ray from where it crosses
    the plane one unit ahead of the eye: of the distance `dist` to the eye the part dist / zc lies before that plane.  Points with
    zc <= 0 lie behind the eye plane; their positions mean nothing."""
    v = np.asarray(P, np.float64) - pin.eye
    zc = v @ pin.ahead
    with np.errstate(all="ignore"):
        sx, sy = (v @ pin.right) / zc, (v @ pin.up) / zc
        fx = (sx / (pin.tan_half * pin.aspect) + 1.0) * 0.5 * W - 0.5
        fy = (1.0 - sy / pin.tan_half) * 0.5 * H - 0.5
        dist = np.sqrt((v * v).sum(-1))
        return fx, fy, zc, dist - dist / zc


# ---- cameras -------------------------------------------------------------------------------------------------------------------------
def _rotate(v, axis, angle):
    axis = _unit(np.asarray(axis, np.float64))
    return v * math.cos(angle) + np.cross(axis, v) * math.sin(angle) + axis * float(axis @ v) * (1.0 - math.cos(angle))


def moved(camera: Camera, right=0.0, up=0.0, ahead=0.0, yaw=0.0, pitch=0.0, roll=0.0, fov_scale=1.0) -> Camera:
    """A copy of `camera` shifted along its own axes (world units), then turned about its up axis (yaw), its right axis (pitch) and its
    viewing direction (roll, through a tilted `up` vector), radians, with the fov scaled."""
    p = pinhole(camera)
    st = camera.state()
    st["eye_pos"] = list(p.eye + right * p.right + up * p.up + ahead * p.ahead)
    d = _rotate(_rotate(p.ahead, p.up, yaw), p.right, pitch)
    st["dir"] = list(d * math.sqrt(float(np.asarray(camera.dir, np.float64) @ np.asarray(camera.dir, np.float64))))
    st["up"] = list(_rotate(p.up, p.ahead, roll))
    st["fov"] = float(F(camera.fov * fov_scale))
    return Camera.from_state(st)


def camera_pairs(fs, W: int, H: int) -> dict:
    """name -> (A, B): the camera the history was rendered from and the current one, both derived from the scene's camera (spheres_room:
    the eye in the middle of a 20 x 11 x 22 room that it looks along, surfaces 7 to 22 units away).
    The base is the scene's camera a little off its place and turned a little about all three axes, at 0.45 of its 90 degree fov:
      - level and on the room's axis, whole rows of the floor share one depth and whole columns one position, so whole rows would sit on
        a cell boundary at once; a dolly along the axis of an odd-sized frame keeps its centre row and column on their pixels (the
        two dollies therefore carry a small sideways step, too);
      - at 90 degrees a pixel of the 29-row frame is 0.069 of the distance wide, a wall's depth changes by more than 2 % per pixel
        almost everywhere and `interior` is nearly empty; at 40.5 degrees a pixel is 0.025 (29 rows) and 0.015 (48 rows) wide.
    A sideways step s moves a surface at distance z by s / (0.015 z) pixels of the 48-row frame, a step d ahead one at image radius r (of
    the plane at distance 1, at most 0.6) by r d / (0.015 (z - d)): the motions of (a), (b), (d) and (e) are sized for 2 to 4 pixels on
    the nearest surfaces.  (c) is larger by necessity: its A stands 0.3 above the floor and 0.4 from the right wall and B steps back
    1.5 units, so that the floor and the wall B sees under and beside itself lie behind A's eye plane; the far wall keeps its history.
      strafe_lift  (a) 0.4 right, 0.25 up
      dolly_in     (b) 1.5 ahead
      dolly_out    (c) 1.5 back, near the floor and the right wall
      turn_zoom    (d) yaw 3.3 and pitch -2.6 pixels, a tilted up vector and fov x 0.85
      all          (e) all of these together (with a step back and a wider fov, so that taps leave the frame on every side)"""
    from tests.helpers import camera_for
    base = moved(camera_for(fs, W, H), right=0.3, up=-0.2, yaw=0.05, pitch=-0.04, roll=0.03, fov_scale=0.45)
    px = 2.0 * math.tan(base.fov / 2.0) / 48.0       # one pixel of the 48-row frame in radians, at the centre
    low = moved(base, right=9.46, up=-4.73, yaw=0.05, pitch=0.04, roll=-0.02)
    return dict(strafe_lift=(base, moved(base, right=0.4, up=0.25)),
                dolly_in=(base, moved(base, ahead=1.5, right=0.04, up=-0.03)),
                dolly_out=(low, moved(low, ahead=-1.5, right=-0.02, up=0.015)),
                turn_zoom=(base, moved(base, yaw=3.3 * px, pitch=-2.6 * px, roll=0.02, fov_scale=0.85)),
                all=(base, moved(base, right=0.3, up=-0.2, ahead=-1.0, yaw=-2.7 * px, pitch=2.2 * px, roll=-0.015, fov_scale=1.0 / 0.85)))


PAIRS = ("strafe_lift", "dolly_in", "dolly_out", "turn_zoom", "all")


def rigid_motion(axis, through, angle, shift) -> np.ndarray:
    """The 4 x 4 float64 matrix of a rotation by `angle` about the line through `through` along `axis`, followed by `shift`."""
    m = np.eye(4)
    m[:3, :3] = np.stack([_rotate(e, axis, angle) for e in np.eye(3)], axis=1)
    c = np.asarray(through, np.float64)
    m[:3, 3] = c - m[:3, :3] @ c + np.asarray(shift, np.float64)
    return m


# ---- the truth of a pair of frames -----------------------------------------------------------------------------------------------------
def _fields(rec):
    rec = np.ascontiguousarray(rec, F).reshape(-1, 8)
    return rec[:, 0:3], rec[:, 3].astype(np.float64), rec[:, 4:7].astype(np.float64), rec[:, 7].view(np.uint32)


def previous_positions(pin_a: Pinhole, pin_b: Pinhole, rec_b, W: int, H: int, rigid=None) -> dict:
    """For every pixel of B's one-sample frame rec_b (n, 8): the world point it shows (the centre ray of B at the record's depth), where
    that point lay when A's frame was rendered -- rigid: {object id: T_prev . T_cur^-1 as a 4 x 4 float64 matrix} for the items that moved
    in between --, and where A's frame shows that place.  -> dict(fx, fy, zc, z_exp (n,) of `inverse`, surface (n,) bool: the record has a
    finite depth and normal (what the call takes for a surface), hit (n,) bool: and that normal has a length (the device marks a miss with
    a NaN normal, the oracle with depth 0 and normal 0: finite, so the call reprojects it, and its zero normal passes no tap), world
    (n, 3), previous (n, 3))."""
    _, depth, normal, ids = _fields(rec_b)
    y, x = np.mgrid[0:H, 0:W]
    o, d = forward(pin_b, x.reshape(-1), y.reshape(-1), W, H)
    surface = np.isfinite(depth) & np.isfinite(normal).all(-1)
    world = o + d * np.where(surface, depth, 1.0)[:, None]
    prev = world.copy()
    for ident, m in (rigid or {}).items():
        at = ids == np.uint32(ident)
        prev[at] = world[at] @ m[:3, :3].T + m[:3, 3]
    fx, fy, zc, z_exp = inverse(pin_a, prev, W, H)
    with np.errstate(invalid="ignore"):
        hit = surface & ((normal * normal).sum(-1) > 0.25)
    return dict(fx=fx, fy=fy, zc=zc, z_exp=z_exp, surface=surface, hit=hit, world=world, previous=prev)


def interior(tr: dict, rec_a, rec_b, W: int, H: int) -> np.ndarray:
    """(n,) bool: the pixels of B whose history is beyond doubt.  The point lies ahead of A; its true previous position lies at least one
    pixel inside A's frame; and every record of A around that position -- the 2 x 2 cell of the position, and of the positions POS_TOL
    to either side, so that a position within rounding of a cell's edge asks for both cells -- has B's object id, a depth within 2 % of
    the expected one and a normal whose dot product with B's is above 0.95.  Every threshold is well inside the call's defaults (5 %,
    0.9): such a pixel must be kept, with four taps or a snap."""
    _, depth_a, normal_a, ids_a = _fields(rec_a)
    _, _, normal_b, ids_b = _fields(rec_b)
    fx, fy, zc, z_exp = tr["fx"], tr["fy"], tr["zc"], tr["z_exp"]
    with np.errstate(invalid="ignore"):
        ok = tr["hit"] & (zc > 0) & (fx >= 1) & (fx <= W - 2) & (fy >= 1) & (fy <= H - 2)
    gx, gy = np.where(ok, fx, 1.0), np.where(ok, fy, 1.0)
    x_lo, x_hi = np.floor(gx - POS_TOL).astype(np.int64), np.floor(gx + POS_TOL).astype(np.int64) + 1
    y_lo, y_hi = np.floor(gy - POS_TOL).astype(np.int64), np.floor(gy + POS_TOL).astype(np.int64) + 1
    for dy in range(3):
        for dx in range(3):
            qx, qy = np.minimum(x_lo + dx, x_hi), np.minimum(y_lo + dy, y_hi)
            q = qy * W + qx
            with np.errstate(invalid="ignore"):
                ok &= (ids_a[q] == ids_b) & (np.abs(depth_a[q] - z_exp) <= 0.02 * z_exp) & ((normal_a[q] * normal_b).sum(-1) > 0.95)
    return ok


def predicted_taps(tr: dict, rec_a, rec_b, W: int, H: int, prm, length_a=None) -> dict:
    """Steps 3 to 6 of rr_accumulate_records' text restated in float64 on the TRUE previous position: which pixels reach the taps
    (alive), which snap, the taps' positions x, y (n, 4) and which are taken (n, 4) (all False where the pixel is not kept: sum_w <
    2^-6), for a history rec_a (n, 8) of finite colours with lengths length_a (default: all 1) and no halves.  prm: a
    temporal.AccumulateParams, its scalars as the float32 values the call sees.
    borderline (n, 4): the float32 arithmetic may decide this tap either way -- the pixel's clip.w, frame bounds, snap decision, cell or
    weight sum lies within POS_TOL pixels (REL_TOL relative for clip.w) of where the decision turns, or the tap's normal or depth test
    within REL_TOL relative of its threshold."""
    colour_b, _, normal_b, ids_b = _fields(rec_b)
    colour_a, depth_a, normal_a, ids_a = _fields(rec_a)
    n = W * H
    length_a = np.ones(n) if length_a is None else np.asarray(length_a, np.float64)
    normal_min, sigma, snap = float(F(prm.normal_min)), float(F(prm.sigma_depth)), float(F(prm.snap))
    fx, fy, zc, z_exp = tr["fx"], tr["fy"], tr["zc"], tr["z_exp"]
    T = POS_TOL
    with np.errstate(invalid="ignore"):
        seen = np.isfinite(colour_b).all(-1) & tr["surface"]
        alive = seen & (zc > EPS) & np.isfinite(fx) & np.isfinite(fy) & (fx > -1) & (fx < W) & (fy > -1) & (fy < H)
        edge = seen & ((np.abs(zc - EPS) <= REL_TOL * EPS) | (np.abs(fx + 1) <= T) | (np.abs(fx - W) <= T) | (np.abs(fy + 1) <= T) | (np.abs(fy - H) <= T))
    gx, gy = np.where(alive, fx, 0.0), np.where(alive, fy, 0.0)
    rx, ry = np.rint(gx), np.rint(gy)
    ax, ay = np.abs(gx - rx), np.abs(gy - ry)
    snapped = (ax <= snap) & (ay <= snap)
    edge |= ((np.abs(ax - snap) <= T) & (ay <= snap + T)) | ((np.abs(ay - snap) <= T) & (ax <= snap + T))
    edge |= ~snapped & ((ax <= T) | (ay <= T))                           # the cell: floor() turns at an integer
    x0 = np.where(snapped, rx, np.floor(gx)).astype(np.int64)
    y0 = np.where(snapped, ry, np.floor(gy)).astype(np.int64)
    tx, ty = np.where(snapped, 0.0, gx - x0), np.where(snapped, 0.0, gy - y0)
    xs, ys = np.zeros((n, 4), np.int64), np.zeros((n, 4), np.int64)
    taken, close, weight = np.zeros((n, 4), bool), np.zeros((n, 4), bool), np.zeros((n, 4))
    for k in range(4):
        qx, qy = x0 + (k & 1), y0 + (k >> 1)
        inside = (qx >= 0) & (qy >= 0) & (qx < W) & (qy < H)
        q = np.where(inside, qy * W + qx, 0)
        with np.errstate(invalid="ignore"):
            dots = (normal_a[q] * normal_b).sum(-1)
            dz, limit = np.abs(z_exp - depth_a[q]), sigma * z_exp + EPS
            t = alive & (k < np.where(snapped, 1, 4)) & inside & (ids_a[q] == ids_b)
            close[:, k] = t & ((np.abs(dots - normal_min) <= REL_TOL * abs(normal_min)) | (np.abs(dz - limit) <= REL_TOL * np.abs(limit)))
            t &= np.isfinite(normal_a[q]).all(-1) & (dots >= normal_min) & np.isfinite(colour_a[q]).all(-1) & np.isfinite(depth_a[q]) & (dz <= limit)
            t &= length_a[q] > 0
        xs[:, k], ys[:, k], taken[:, k] = qx, qy, t
        weight[:, k] = (tx if k & 1 else 1.0 - tx) * (ty if k >> 1 else 1.0 - ty)
    sum_w = (weight * taken).sum(1)
    kept = alive & (sum_w >= MIN_WEIGHT)
    edge |= alive & (np.abs(sum_w - MIN_WEIGHT) <= 4 * T)                # a position T off moves a sum of weights by at most 2 T per axis
    return dict(alive=alive, snapped=snapped & alive, kept=kept, x=xs, y=ys, weight=weight, taken=taken & kept[:, None],
                borderline=close | edge[:, None], pixel_borderline=edge, n_taps=np.where(alive, np.where(snapped, 1, 4), 0))


# ---- the inputs that make a call's output its tap position, and what is asked of that output -----------------------------------------------
def ramp_inputs(rec_a, rec_b, W: int, H: int, checker: bool = False) -> dict:
    """The arguments of the four accumulation calls (as the yardsticks name them) over A's frame rec_a as the history and B's frame rec_b
    as the current one, with colours that make the output the position: every history colour -- records, both halves, diffuse and its
    halves -- is (x of the pixel, y of the pixel, A's depth), every history length 1 and every current colour 0 (checker: 0 or 1 by the
    parity of x + y, for the clamped calls, whose boxes then have a spread everywhere).  A kept pixel has N = 2 exactly, its output is
    h + 0.5 (cur - h), and 2 out - cur is the history mean h: the weighted mean of the taps' positions."""
    n = W * H
    rec_a, rec_b = np.ascontiguousarray(rec_a, F).reshape(n, 8), np.ascontiguousarray(rec_b, F).reshape(n, 8)
    y, x = np.mgrid[0:H, 0:W]
    ramp = np.stack([x.reshape(-1), y.reshape(-1), np.where(np.isfinite(rec_a[:, 3]), rec_a[:, 3], 0)], axis=-1).astype(F)
    cur = np.repeat((((x + y) & 1).reshape(-1, 1) if checker else np.zeros((n, 1))).astype(F), 3, axis=1)
    history, records = rec_a.copy(), rec_b.copy()
    history[:, 0:3], records[:, 0:3] = ramp, cur
    two = lambda a: np.ascontiguousarray(np.stack([a, a], axis=1))
    d = dict(records=records, halves=two(records), diffuse=cur.copy(), diffuse_halves=two(cur), history=history, history_halves=two(history),
             history_diffuse=ramp.copy(), history_diffuse_halves=two(ramp), history_length=np.ones(n, F), current=cur)
    for v in d.values():
        v.setflags(write=False)
    return d


def history_means(out: dict, current) -> dict:
    """layer name -> (n, 3) float64, 2 out - current of every colour layer an accumulation call returned."""
    cur = np.asarray(current, np.float64)
    h = lambda a: 2.0 * np.asarray(a, np.float64) - cur
    layers = dict(records=h(np.asarray(out["records"])[:, 0:3]))
    if out.get("halves") is not None:
        layers.update(half0=h(np.asarray(out["halves"])[:, 0, 0:3]), half1=h(np.asarray(out["halves"])[:, 1, 0:3]))
    if out.get("diffuse") is not None:
        layers["diffuse"] = h(out["diffuse"])
    if out.get("diffuse_halves") is not None:
        layers.update(diffuse_half0=h(np.asarray(out["diffuse_halves"])[:, 0]), diffuse_half1=h(np.asarray(out["diffuse_halves"])[:, 1]))
    return layers


def position_errors(mean_xy, tr: dict, pred: dict, length) -> dict:
    """One layer's history mean (n, 2) against the truth.  four: the pixels the float64 gate keeps with all four taps, no decision of theirs
    borderline; snap: those it snaps.  -> dict(four, snap (n,) bool, bad_four, bad_snap (n,) bool: the pixel has no history of length 2, or
    (four) its mean lies further than POS_TOL from the true position, (snap) its mean is not the nearest pixel exactly or the true
    position lies further than snap + POS_TOL from it; worst: the largest error over `four` in pixels)."""
    sure = ~pred["borderline"].any(1)
    four = sure & pred["kept"] & ~pred["snapped"] & pred["taken"].all(1)
    snap = sure & pred["kept"] & pred["snapped"] & pred["taken"][:, 0]
    truth = np.stack([tr["fx"], tr["fy"]], axis=-1)
    with np.errstate(invalid="ignore"):
        err = np.abs(np.asarray(mean_xy, np.float64) - truth).max(-1)
        near = np.rint(truth)
        two = np.asarray(length) == 2
        bad_four = four & ~(two & (err <= POS_TOL))
        bad_snap = snap & ~(two & (np.asarray(mean_xy, np.float64) == near).all(-1))
    return dict(four=four, snap=snap, bad_four=bad_four, bad_snap=bad_snap, worst=float(err[four & two].max()) if (four & two).any() else 0.0)


def no_history(tr: dict, W: int, H: int) -> tuple:
    """(behind, outside) (n,) bool: B's pixels that hit a surface whose point lies behind A's eye plane (true zc <= 0), and those ahead of it whose true
    previous position lies outside (-1, W) x (-1, H) by more than OUTSIDE_TOL pixels.  Neither can have history."""
    fx, fy, zc = tr["fx"], tr["fy"], tr["zc"]
    with np.errstate(invalid="ignore"):
        behind = tr["hit"] & (zc <= 0)
        t = OUTSIDE_TOL
        outside = tr["hit"] & (zc > 0) & ((fx < -1 - t) | (fx > W + t) | (fy < -1 - t) | (fy > H + t))
    return behind, outside


def check_outputs(out: dict, inputs: dict, tr: dict, pred: dict, inside: np.ndarray, W: int, H: int, snap_width: float, what: str) -> dict:
    """Everything that is asked of ONE accumulation call's outputs (the yardstick's, the host loop's or the device's) on ramp_inputs,
    asserted: position and snap on every colour layer, completeness on `inside` (interior's pixels), no history behind and outside.
    -> dict(worst position error in pixels, four, snapped: how many pixels each)."""
    length = np.asarray(out["length"])
    worst, res = 0.0, None
    for name, mean in history_means(out, inputs["current"]).items():
        res = position_errors(mean[:, 0:2], tr, pred, length)
        assert not res["bad_four"].any(), f"{what}, {name}: {int(res['bad_four'].sum())} of {int(res['four'].sum())} four-tap pixels off their true position"
        assert not res["bad_snap"].any(), f"{what}, {name}: {int(res['bad_snap'].sum())} of {int(res['snap'].sum())} snapped pixels off"
        worst = max(worst, res["worst"])
    truth = np.stack([tr["fx"], tr["fy"]], axis=-1)
    with np.errstate(invalid="ignore"):
        assert (np.abs(truth - np.rint(truth)).max(-1)[res["snap"]] <= snap_width + POS_TOL).all(), what
    # completeness: an interior pixel is kept, and its mean is the true position (a tap left out would pull it off) or the snap's pixel
    mean = history_means(out, inputs["current"])["records"][:, 0:2]
    with np.errstate(invalid="ignore"):
        placed = (np.abs(mean - truth).max(-1) <= POS_TOL) | ((mean == np.rint(truth)).all(-1) & (np.abs(truth - np.rint(truth)).max(-1) <= snap_width + POS_TOL))
    lost = inside & ~((length == 2) & placed)
    assert not lost.any(), f"{what}: {int(lost.sum())} of {int(inside.sum())} interior pixels lost their history or a tap"
    behind, outside = no_history(tr, W, H)
    gone = behind | outside
    assert (length[gone] == 1).all(), f"{what}: {int((length[gone] != 1).sum())} pixels behind or outside the previous view kept a history"
    for key in ("records", "halves", "diffuse", "diffuse_halves"):
        if out.get(key) is not None:
            got, cur = np.ascontiguousarray(out[key], F).reshape(W * H, -1), np.ascontiguousarray(inputs[key], F).reshape(W * H, -1)
            assert np.array_equal(got[gone].view(np.uint32), cur[gone].view(np.uint32)), f"{what}: {key} of a pixel without history is not its current bits"
    return dict(worst=worst, four=int(res["four"].sum()), snapped=int(res["snap"].sum()))


# ---- frames ----------------------------------------------------------------------------------------------------------------------------
def frame_config():
    from rustray_amd.flat import make_config
    return make_config(samples=1, monte_carlo=False, max_recursion=0)


def pack(color, depth, normal, object_id) -> np.ndarray:
    rec = np.zeros((np.asarray(depth).size, 8), F)
    rec[:, 0:3], rec[:, 3], rec[:, 4:7] = np.asarray(color, F).reshape(-1, 3), np.asarray(depth, F).reshape(-1), np.asarray(normal, F).reshape(-1, 3)
    rec[:, 7] = np.asarray(object_id, np.uint32).reshape(-1).view(F)
    return rec


def oracle_records(oracle, fs, camera) -> np.ndarray:
    """The oracle's one-sample frame of `camera` as (n, 8) records of its means (colour, depth and normal are the one sample's own)."""
    r = oracle.render(fs.c_struct(), camera.c_struct(), frame_config(), n_threads=4, want_means=True)
    return pack(r["mean_rgb"], r["mean_depth"], r["mean_normal"], r["object_id"])


# ---- the moved items of the motion case ------------------------------------------------------------------------------------------------
MOVED_NAMES = ("sphere_texture", "mesh_back")


@functools.lru_cache(maxsize=None)
def _moves():
    return (rigid_motion((0.2, 1.0, 0.1), (2.5, 0.0, -9.0), 0.03, (0.25, 0.1, -0.15)),      # the sphere at (0, -1, -10): an axis 2.7 units off its centre
            rigid_motion((0.0, 1.0, 0.3), (-8.0, 0.0, -12.0), -0.012, (0.0, 0.12, 0.4)))    # the wall z = -20: an axis eight units in front of it, left of the middle


def moved_scene(fs):
    """spheres_room with one sphere and one wall moved between A's frame and B's by a rotation about an axis off their centre plus a shift.
    -> (the scene B sees, item indices (2,), prev_trans (2, 4, 4) float32: their `trans` in A's frame, (trans, trans_inv) (n_items, 4, 4)
    float32 of B's scene, rigid: {object id: T_prev . T_cur^-1 float64, from the float32 matrices the calls see})."""
    from tests.helpers import item_transforms, with_transforms
    t, ti = item_transforms(fs)
    t, ti = t.copy(), ti.copy()
    index = [next(k for k, it in enumerate(fs.items) if it.name == name) for name in MOVED_NAMES]
    prev = t[index].copy()
    rigid = {}
    for k, m in zip(index, _moves()):
        cur = m @ t[k].astype(np.float64)
        t[k], ti[k] = cur.astype(F), np.linalg.inv(cur).astype(F)
        rigid[int(fs.items[k].id)] = prev[len(rigid)].astype(np.float64) @ ti[k].astype(np.float64)
    return with_transforms(fs, t, ti), np.array(index, np.uint32), prev, (t, ti), rigid
