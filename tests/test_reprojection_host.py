"""The temporal reprojection against float64 geometry with the camera moving, without a GPU: the four numpy yardsticks of
rustray_amd/temporal.py (which the kernels and the host loop equal bit for bit) on the oracle's one-sample frames of spheres_room from two
cameras, held to tests/reprojection_truth.py -- a pinhole model written from the camera's definition, itself pinned to the oracle's
primary ray.  What the bit-for-bit tests cannot see is seen here: pixel centres and the y flip, the ray origin one unit ahead of the eye,
the tap order, the matrix order, which view is the previous one.

One sample per pixel and no depth of field: with more samples the mean depth is not the centre ray's depth and the position error is a
property of the design, not a bug (reprojection_truth's docstring).

Figures of this module on the oracle's frames (the tests print them; DESIGN.md section 8, item 27, has the table per pair and size, the
device's beside them): the largest position error is 1.39e-5 px at 64x48 and 1.11e-5 px at 37x29 against the bound 2^-14 = 6.1e-5; the
interior pixels are 17.7 % to 68.5 % of the pixels that hit a surface (156 at the least); at most 0.093 % of the taps are borderline."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from rustray_amd import temporal
from rustray_amd.pixel_rays import pixel_rays
from rustray_amd.temporal import AccumulateParams, HistoryClampParams, previous_view
from tests import reprojection_truth as rt
from tests import temporal_host_loop
from tests.denoise_cases import same_bits
from tests.helpers import load_scene

F = np.float32
CASES = [(pair, size) for pair in rt.PAIRS for size in rt.SIZES]
IDS = [f"{pair}-{size[0]}x{size[1]}" for pair, size in CASES]
KEYS = ("records", "halves", "history", "history_halves", "history_length")
SPLIT_KEYS = ("records", "halves", "diffuse", "diffuse_halves", "history", "history_halves", "history_diffuse", "history_diffuse_halves", "history_length")
_cases = {}


def make_case(oracle, pair, size, frames=None):
    """Everything the tests of one pair and size share, made once and left unchanged: the cameras, their frames (the oracle's, or
    frames(fs, camera) -> records), the truth, the float64 gate, the interior pixels, the ramp inputs and the call's parameters."""
    W, H = size
    fs = load_scene("spheres_room")
    A, B = rt.camera_pairs(fs, W, H)[pair]
    render = frames or (lambda scene, camera: rt.oracle_records(oracle, scene, camera))
    rec_a, rec_b = render(fs, A), render(fs, B)
    m, eye = previous_view(A)
    prm = AccumulateParams(prev_world_to_clip=m, prev_eye=eye)
    tr = rt.previous_positions(rt.pinhole(A), rt.pinhole(B), rec_b, W, H)
    return dict(W=W, H=H, fs=fs, A=A, B=B, rec_a=rec_a, rec_b=rec_b, prm=prm, tr=tr, pred=rt.predicted_taps(tr, rec_a, rec_b, W, H, prm),
                inside=rt.interior(tr, rec_a, rec_b, W, H), inputs=rt.ramp_inputs(rec_a, rec_b, W, H), checker=rt.ramp_inputs(rec_a, rec_b, W, H, checker=True))


@pytest.fixture(scope="module")
def case(oracle):
    def get(pair, size):
        if (pair, size) not in _cases:
            _cases[pair, size] = make_case(oracle, pair, size)
        return _cases[pair, size]
    return get


def conditions(c, pair, what):
    """What makes a case worth its checks, asserted: enough interior pixels, few borderline taps, and for dolly_out pixels behind A."""
    tr, pred, inside = c["tr"], c["pred"], c["inside"]
    surface = int(tr["hit"].sum())
    share = inside.sum() / surface
    taps = int(pred["n_taps"].sum())
    k = np.arange(4)[None, :] < pred["n_taps"][:, None]
    borderline = float((pred["borderline"] & k).sum() / taps)
    behind, outside = rt.no_history(tr, c["W"], c["H"])
    print(f"{what}: {int(inside.sum())} interior pixels, {100 * share:.1f} % of {surface} surface pixels; {100 * borderline:.3f} % of {taps} taps borderline; "
          f"{int(behind.sum())} pixels behind the previous eye plane, {int(outside.sum())} outside its frame")
    assert share >= 0.10 and inside.sum() >= 100, what
    assert borderline <= 0.01, what
    if pair == "dolly_out":
        assert behind.sum() >= 20, what
    return dict(interior=int(inside.sum()), share=share, borderline=borderline, behind=int(behind.sum()), outside=int(outside.sum()))


# ---- the model -------------------------------------------------------------------------------------------------------------------------
def _oracle_rays(oracle, cam_struct):
    fn = oracle.lib().rro_primary_ray
    fn.restype = None
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint16, C.c_uint16, C.c_void_p, C.c_void_p]
    cfg = rt.frame_config()
    (xi, yi), = [(int(a), int(b)) for a, b in oracle.sample_table(1)[0]]
    W, H = int(cam_struct.width), int(cam_struct.height)
    o, d = np.zeros((W * H, 3), F), np.zeros((W * H, 3), F)
    for p in range(W * H):
        fn(C.addressof(cam_struct), C.addressof(cfg), p % W, p // W, xi, yi, o.ctypes.data + 12 * p, d.ctypes.data + 12 * p)
    return o, d


@pytest.mark.parametrize("pair,size", CASES, ids=IDS)
def test_the_model_is_the_oracles_primary_ray(oracle, case, pair, size):
    """forward() at the pixel centres against the oracle's own primary ray (the reference's restatement; its direction normalised in
    float64) and against pixel_rays, for both cameras: within 4 float32 ulps of the largest coordinate.  This pins the truth to the
    reference, not to the code under test."""
    c = case(pair, size)
    W, H = size
    y, x = np.mgrid[0:H, 0:W]
    for name in "AB":
        o, d = rt.forward(rt.pinhole(c[name]), x.reshape(-1), y.reshape(-1), W, H)
        cs = c[name].c_struct()
        ro, rd = _oracle_rays(oracle, cs)
        rd = rd.astype(np.float64) / np.sqrt((rd.astype(np.float64) ** 2).sum(-1))[:, None]
        po, pd = pixel_rays(c[name])
        for what, got, want in (("oracle origins", o, ro), ("oracle directions", d, rd), ("pixel_rays origins", o, po), ("pixel_rays directions", d, pd)):
            bound = 4 * float(np.spacing(F(np.abs(want).max())))
            err = float(np.abs(got - want).max())
            print(f"{pair} {W}x{H} camera {name}, {what}: {err:.3g} (bound {bound:.3g})")
            assert err <= bound, (name, what)


def test_inverse_undoes_forward():
    fs = load_scene("spheres_room")
    A, B = rt.camera_pairs(fs, 37, 29)["all"]
    rng = np.random.default_rng(5)
    fx, fy, t = rng.uniform(-3, 40, 500), rng.uniform(-3, 32, 500), rng.uniform(0.5, 30, 500)
    for cam in (A, B):
        pin = rt.pinhole(cam)
        o, d = rt.forward(pin, fx, fy, 37, 29)
        gx, gy, zc, z = rt.inverse(pin, o + d * t[:, None], 37, 29)
        assert np.abs(gx - fx).max() < 1e-10 and np.abs(gy - fy).max() < 1e-10 and np.abs(z - t).max() < 1e-10 and (zc > 1).all()
    # row 0 is the top row and column 0 the left one: a point up and to the right of the axis lies right of and above the centre
    pin = rt.pinhole(A)
    gx, gy, zc, _ = rt.inverse(pin, pin.eye + 5 * pin.ahead + pin.right + pin.up, 37, 29)
    assert gx > 18 and gy < 14 and abs(zc - 5) < 1e-12


# ---- position, completeness, the gate ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair,size", CASES, ids=IDS)
def test_position_completeness_and_gate(case, pair, size):
    c = case(pair, size)
    W, H = size
    what = f"{pair} {W}x{H}"
    conditions(c, pair, what)
    i, tr, pred = c["inputs"], c["tr"], c["pred"]
    got = temporal.accumulate_records(*(i[k] for k in KEYS), None, c["B"], c["prm"])
    res = rt.check_outputs(got, i, tr, pred, c["inside"], W, H, c["prm"].snap, what)
    print(f"{what}: largest position error {res['worst']:.3g} px over {res['four']} four-tap pixels (bound {rt.POS_TOL:.3g}); {res['snapped']} snapped")
    assert res["four"] >= 100
    # the yardstick's own account of its taps: the same positions, and every interior pixel with four taps or a snap
    taps = got["taps"]
    w = np.where(taps["taken"], taps["weight"].astype(np.float64), 0.0)
    with np.errstate(invalid="ignore"):
        mean = np.stack([(w * taps["x"]).sum(1), (w * taps["y"]).sum(1)], axis=-1) / w.sum(1)[:, None]
    acc = rt.position_errors(mean, tr, pred, got["length"])
    assert not acc["bad_four"].any() and not acc["bad_snap"].any(), what
    full = taps["taken"].all(1) | (taps["taken"][:, 0] & (taps["weight"][:, 0] == 1))
    assert full[c["inside"]].all() and (got["length"][c["inside"]] == 2).all(), what
    # the gate: on every tap that no rounding can turn, the yardstick decides as the float64 restatement does on the true position
    sure = ~pred["borderline"]
    assert np.array_equal(taps["taken"][sure], pred["taken"][sure]), f"{what}: {int((taps['taken'] != pred['taken'])[sure].sum())} taps decided otherwise"
    live = pred["alive"] & ~pred["pixel_borderline"]
    assert np.array_equal(taps["reprojected"][~pred["pixel_borderline"]], pred["alive"][~pred["pixel_borderline"]])
    k = np.arange(4)[None, :] < pred["n_taps"][:, None]
    assert np.array_equal(taps["x"][live[:, None] & k], pred["x"][live[:, None] & k]) and np.array_equal(taps["y"][live[:, None] & k], pred["y"][live[:, None] & k])
    assert set(np.unique(got["length"])) <= {1.0, 2.0}


def test_taps_leave_the_frame_through_all_four_edges(case):
    for size in rt.SIZES:
        W, H = size
        left = right = top = bottom = 0
        for pair in rt.PAIRS:
            pred = case(pair, size)["pred"]
            k = pred["alive"][:, None] & (np.arange(4)[None, :] < pred["n_taps"][:, None])
            left, right = left + int((pred["x"][k] < 0).sum()), right + int((pred["x"][k] >= W).sum())
            top, bottom = top + int((pred["y"][k] < 0).sum()), bottom + int((pred["y"][k] >= H).sum())
        print(f"{W}x{H}: taps off the left {left}, right {right}, top {top}, bottom {bottom}")
        assert min(left, right, top, bottom) >= 1


# ---- all four yardsticks, every layer ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair,size", CASES, ids=IDS)
def test_every_yardstick_and_every_layer(case, pair, size):
    c = case(pair, size)
    W, H = size
    i, k, tr, pred = c["inputs"], c["checker"], c["tr"], c["pred"]
    plain = temporal.accumulate_records(*(i[key] for key in KEYS), None, c["B"], c["prm"])
    split = temporal.accumulate_split_records(*(i[key] for key in SPLIT_KEYS), None, c["B"], c["prm"])
    worst = [rt.check_outputs(split, i, tr, pred, c["inside"], W, H, c["prm"].snap, f"{pair} {W}x{H} split")["worst"]]
    assert same_bits(split["records"], plain["records"]) and same_bits(split["length"], plain["length"])
    for radius in (1, 2):
        clamp = HistoryClampParams(radius=radius, sigma_scale=65536.0)
        for name, got in (("clamped", temporal.accumulate_clamped_records(*(k[key] for key in KEYS), None, c["B"], c["prm"], clamp)),
                          ("clamped split", temporal.accumulate_clamped_split_records(*(k[key] for key in SPLIT_KEYS), None, c["B"], c["prm"], clamp))):
            what = f"{pair} {W}x{H} {name} radius {radius}"
            assert not got["clamped"].any() and not got.get("diffuse_clamped", np.zeros(1, bool)).any(), what       # no box is reached ...
            assert set(np.unique(got["length"])) <= {1.0, 2.0} and same_bits(got["length"], plain["length"]), what  # ... so no length is shortened
            worst.append(rt.check_outputs(got, k, tr, pred, c["inside"], W, H, c["prm"].snap, what)["worst"])
    print(f"{pair} {W}x{H}: largest position error {max(worst):.3g} px over all four calls and every layer (bound {rt.POS_TOL:.3g})")


# ---- motion and camera together ---------------------------------------------------------------------------------------------------------
def make_motion_case(oracle, size, frames=None):
    """Pair (a) with one sphere and one wall moved between the two frames (reprojection_truth.moved_scene)."""
    W, H = size
    fs = load_scene("spheres_room")
    A, B = rt.camera_pairs(fs, W, H)["strafe_lift"]
    fs_b, index, prev, (t, ti), rigid = rt.moved_scene(fs)
    render = frames or (lambda scene, camera: rt.oracle_records(oracle, scene, camera))
    rec_a, rec_b = render(fs, A), render(fs_b, B)
    m, eye = previous_view(A)
    prm = AccumulateParams(prev_world_to_clip=m, prev_eye=eye)
    tr = rt.previous_positions(rt.pinhole(A), rt.pinhole(B), rec_b, W, H, rigid)
    ids = np.array([fs.items[k].id for k in index], np.uint32)
    return dict(W=W, H=H, fs=fs, fs_b=fs_b, A=A, B=B, rec_a=rec_a, rec_b=rec_b, prm=prm, tr=tr, pred=rt.predicted_taps(tr, rec_a, rec_b, W, H, prm),
                inside=rt.interior(tr, rec_a, rec_b, W, H), inputs=rt.ramp_inputs(rec_a, rec_b, W, H), index=index, prev=prev, trans=(t, ti), ids=ids,
                on_moved=np.isin(rec_b[:, 7].view(np.uint32), ids))


def moved_conditions(c, what):
    """Asserted: the moved items cover enough of B's frame, enough of it interior, and their motion is what decides the position."""
    on, inside = c["on_moved"], c["inside"]
    still = rt.previous_positions(rt.pinhole(c["A"]), rt.pinhole(c["B"]), c["rec_b"], c["W"], c["H"])
    with np.errstate(invalid="ignore"):
        shift = np.hypot(c["tr"]["fx"] - still["fx"], c["tr"]["fy"] - still["fy"])[on & c["tr"]["hit"]]
    print(f"{what}: {int(on.sum())} pixels on the moved items, {int((on & inside).sum())} of them interior; their motion is {shift.min():.2f} to {shift.max():.2f} px")
    assert (on & inside).sum() >= 50 and (on & inside).sum() >= 0.1 * on.sum() and shift.min() > 100 * rt.POS_TOL, what
    for ident in c["ids"]:
        assert (inside & (c["rec_b"][:, 7].view(np.uint32) == ident)).sum() >= 10, (what, int(ident))


@pytest.mark.parametrize("size", rt.SIZES, ids=[f"{w}x{h}" for w, h in rt.SIZES])
def test_motion_and_camera_together(oracle, size):
    """A rotated and shifted sphere and wall under the strafing camera: motion_records -> accumulate_records against
    inverse(A, T_prev . T_cur^-1 . P), with the position and completeness checks on every pixel, the moved items' among them."""
    c = make_motion_case(oracle, size)
    W, H = size
    what = f"moved items {W}x{H}"
    moved_conditions(c, what)
    t, ti = c["trans"]
    motion, _ = temporal.motion_records(c["inputs"]["records"], c["B"], c["ids"], c["prev"], ti[c["index"]])
    assert (motion[c["on_moved"]] != 0).any(-1).all() and not motion[~c["on_moved"]].any()
    got = temporal.accumulate_records(*(c["inputs"][k] for k in KEYS), motion, c["B"], c["prm"])
    res = rt.check_outputs(got, c["inputs"], c["tr"], c["pred"], c["inside"], W, H, c["prm"].snap, what)
    on = rt.position_errors(rt.history_means(got, c["inputs"]["current"])["records"][:, 0:2], c["tr"], c["pred"], got["length"])
    print(f"{what}: largest position error {res['worst']:.3g} px; {int((on['four'] & c['on_moved']).sum())} four-tap pixels on the moved items")
    assert (on["four"] & c["on_moved"]).sum() >= 50
    # and without the motion the moved items' pixels are off: the check sees the motion
    blind = temporal.accumulate_records(*(c["inputs"][k] for k in KEYS), None, c["B"], c["prm"])
    off = rt.position_errors(rt.history_means(blind, c["inputs"]["current"])["records"][:, 0:2], c["tr"], c["pred"], blind["length"])
    assert off["bad_four"][on["four"] & c["on_moved"]].all()


# ---- negative controls ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", rt.PAIRS)
def test_the_bounds_can_fail(case, pair):
    """Three mistakes of the kind the bounds exist for, each fed to the yardstick through its parameters: A's eye 0.001 units off, B's own
    view taken for the previous one, the matrix transposed.  Each puts at least half of the four-tap pixels off their true position."""
    c = case(pair, rt.SIZES[0])
    i = c["inputs"]
    m_off, eye_off = previous_view(rt.moved(c["A"], right=0.001))
    m_b, eye_b = previous_view(c["B"])
    wrong = dict(eye=dataclasses.replace(c["prm"], prev_world_to_clip=m_off, prev_eye=eye_off), own_view=dataclasses.replace(c["prm"], prev_world_to_clip=m_b, prev_eye=eye_b),
                 transposed=dataclasses.replace(c["prm"], prev_world_to_clip=np.ascontiguousarray(np.asarray(c["prm"].prev_world_to_clip).T)))
    for name, prm in wrong.items():
        got = temporal.accumulate_records(*(i[k] for k in KEYS), None, c["B"], prm)
        res = rt.position_errors(rt.history_means(got, i["current"])["records"][:, 0:2], c["tr"], c["pred"], got["length"])
        share = res["bad_four"].sum() / res["four"].sum()
        print(f"{pair}, {name}: {100 * share:.1f} % of {int(res['four'].sum())} four-tap pixels fail the position check")
        assert share >= 0.5, (pair, name)


# ---- the host loop ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return temporal_host_loop.build(tmp_path_factory)


@pytest.mark.parametrize("size", rt.SIZES, ids=[f"{w}x{h}" for w, h in rt.SIZES])
def test_the_host_loop_on_the_moving_camera(case, host_exe, tmp_path, size):
    """The C++ temporal_pixel<> (tests/temporal_host_loop.py) on pair (e): every word the yardstick's, plain and clamped split; and the
    checks on what it wrote."""
    exe = host_exe
    c = case("all", size)
    i, k = c["inputs"], c["checker"]
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    got = temporal_host_loop.run(exe, tmp_path, c["B"], c["prm"], None, False, tuple(i[key] for key in KEYS) + (None,))
    want = temporal.accumulate_records(*(i[key] for key in KEYS), None, c["B"], c["prm"])
    for key in ("records", "halves", "length"):
        assert np.array_equal(bits(got[key]), bits(want[key])), key
    clamp = HistoryClampParams(radius=2, sigma_scale=65536.0)
    got = temporal_host_loop.run(exe, tmp_path, c["B"], c["prm"], clamp, True, tuple(k[key] for key in SPLIT_KEYS) + (None,))
    want = temporal.accumulate_clamped_split_records(*(k[key] for key in SPLIT_KEYS), None, c["B"], c["prm"], clamp)
    for key in ("records", "halves", "length", "diffuse", "diffuse_halves"):
        assert np.array_equal(bits(got[key]), bits(want[key])), key
    rt.check_outputs(got, k, c["tr"], c["pred"], c["inside"], *size, c["prm"].snap, f"host loop {size}")
