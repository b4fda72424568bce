"""The temporal reprojection of rr_accumulate_records without a GPU: the host loop over rustray_amd/csrc/rr_temporal.h (the functions the
kernel applies per lane) under AddressSanitizer + UBSan against the numpy yardstick rustray_amd/temporal.py, bit for bit; the yardstick's
own properties (a static camera, the incremental mean, a disocclusion); and what the entry points refuse before they touch a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from rustray_amd import capi, temporal
from rustray_amd.temporal import AccumulateParams, accumulate_records
from tests import temporal_host_loop
from tests.denoise_cases import F, same_bits
from tests.helpers import ROOT, host_api_source
from tests.temporal_cases import boundary_frames, frame_params, static_frames, temporal_frame

NEW = ("rr_accumulate_default_params", "rr_accumulate_records_device", "rr_accumulate_records")


@pytest.fixture(scope="module")
def host_loop(tmp_path_factory):
    exe = temporal_host_loop.build(tmp_path_factory)

    def run(tmp_path, cam, prm, records, halves, history, history_halves, history_length, motion):
        return temporal_host_loop.run(exe, tmp_path, cam, prm, None, False,
                                      (records, halves, history, history_halves if halves is not None else None, history_length, motion))
    return run


def _same(got, want, what):
    for key in ("records", "length", "halves"):
        if want[key] is None:
            assert got[key] is None
            continue
        g, w = np.ascontiguousarray(got[key]).view(np.uint32), np.ascontiguousarray(want[key]).view(np.uint32)
        assert same_bits(g, w), f"{what}: {int((g != w).sum())} words of {key} differ"


def _inputs(case, use_halves, use_motion, first):
    hv = case["halves"] if use_halves else None
    if first:
        return case["records"], hv, None, None, None, case["motion"] if use_motion else None
    return case["records"], hv, case["history"], case["history_halves"] if use_halves else None, case["history_length"], case["motion"] if use_motion else None


def test_the_generated_case_has_what_it_promises():
    case = temporal_frame(37, 19)
    W, H = 37, 19
    rec, hist = case["records"], case["history"]
    assert np.isnan(rec[:, 0]).any() and np.isinf(rec[:, 2]).any() and np.isnan(rec[:, 4]).any()
    assert (~np.isfinite(hist[:, 0:3])).any() and (~np.isfinite(case["history_halves"][:, :, 0:3])).any() and (case["history_length"] == 0).any()
    assert (case["motion"] != 0).any() and len(np.unique(rec[:, 7].view(np.uint32))) >= 5
    got = accumulate_records(rec, case["halves"], hist, case["history_halves"], case["history_length"], None, case["cam"], frame_params(case, snap=0.0))
    taps, kept = got["taps"], got["length"] > 1
    # taps off every edge of the frame, among the pixels that were reprojected at all
    live = taps["reprojected"]
    assert (taps["x"][live] < 0).any() and (taps["x"][live] >= W).any() and (taps["y"][live] < 0).any() and (taps["y"][live] >= H).any()
    # the pixel behind the previous eye has no history; plenty of pixels keep theirs, plenty do not
    assert got["length"][(H // 2) * W + W // 2] == 1
    assert 0.1 < kept.mean() < 0.9, kept.mean()
    # the previous view is about 1.3 pixels off: the kept pixels use bilinear taps
    assert (taps["taken"].sum(1)[kept] > 1).any()


@pytest.mark.parametrize("size", [(37, 19), (130, 70)])
@pytest.mark.parametrize("use_halves,use_motion,snap,first", [
    (True, True, 1 / 64, False), (True, False, 0.0, False), (False, True, 0.0, False), (False, False, 1 / 64, False),
    (True, True, 1 / 64, True), (False, False, 0.0, True),
])
def test_host_loop_equals_the_yardstick(host_loop, tmp_path, size, use_halves, use_motion, snap, first):
    case = temporal_frame(*size)
    prm = frame_params(case, snap=snap)
    args = _inputs(case, use_halves, use_motion, first)
    want = accumulate_records(*args, case["cam"], prm)
    _same(host_loop(tmp_path, case["cam"], prm, *args), want, f"{size} halves={use_halves} motion={use_motion} snap={snap} first={first}")
    if first:
        assert same_bits(want["records"], case["records"]) and set(np.unique(want["length"])) == {0.0, 1.0}


def test_host_loop_equals_the_yardstick_on_the_static_view(host_loop, tmp_path):
    cam, prm, records, halves = static_frames(37, 19, 2)
    first = accumulate_records(records[0], halves[0], None, None, None, None, cam, prm)
    args = (records[1], halves[1], first["records"], first["halves"], first["length"], None)
    _same(host_loop(tmp_path, cam, prm, *args), accumulate_records(*args, cam, prm), "static view")


# ---- properties of the yardstick ------------------------------------------------------------------------------------------------
def _feed(cam, prm, frames, halves=None):
    state = dict(records=None, halves=None, length=None)
    for k, rec in enumerate(frames):
        state = accumulate_records(rec, None if halves is None else halves[k], state["records"], state["halves"], state["length"], None, cam, prm)
        yield state


@pytest.mark.parametrize("size", [(37, 19), (130, 70)])
def test_a_static_camera_snaps_every_pixel_to_itself(size):
    """The condition that makes the static cases meaningful: with the camera's own matrices as the previous view every valid pixel's
    reprojection lies within snap = 1/64 of its own centre, and its one tap is taken."""
    W, H = size
    cam, prm, records, halves = static_frames(W, H, 2)
    first = accumulate_records(records[0], None, None, None, None, None, cam, prm)
    taps = accumulate_records(records[1], None, first["records"], None, first["length"], None, cam, prm)["taps"]
    p = np.arange(W * H)
    assert (taps["x"][:, 0] == p % W).all() and (taps["y"][:, 0] == p // W).all()
    assert (taps["weight"][:, 0] == 1).all() and taps["taken"][:, 0].all() and not taps["taken"][:, 1:].any()


def test_a_static_camera_keeps_a_repeated_frame_bit_for_bit():
    cam, prm, records, halves = static_frames(37, 19, 1)
    for k, state in enumerate(_feed(cam, prm, [records[0]] * 40, [halves[0]] * 40), start=1):
        assert same_bits(state["records"], records[0]) and same_bits(state["halves"], halves[0]), k
        assert (state["length"] == min(k, 32)).all(), k


def test_a_static_camera_forms_the_mean_of_its_frames():
    """h + (c - h) / N over N = 1 .. 8 is the running mean; every step rounds a division, a difference, a product and a sum, each by at
    most 2^-24 of the largest colour: well inside 8 * 2^-22 * max|c| of the float64 mean."""
    cam, prm, records, halves = static_frames(37, 19, 8)
    state = list(_feed(cam, prm, records, halves))[-1]
    assert (state["length"] == 8).all()
    for got, frames in ((state["records"][:, 0:3], records[:, :, 0:3]), (state["halves"][:, 0, 0:3], halves[:, :, 0, 0:3]),
                        (state["halves"][:, 1, 0:3], halves[:, :, 1, 0:3])):
        mean = frames.astype(np.float64).mean(0)
        bound = 8 * 2.0 ** -22 * float(np.abs(frames).max())
        err = float(np.abs(got.astype(np.float64) - mean).max())
        print(f"largest deviation from the float64 mean {err:.3g}, bound {bound:.3g}")
        assert err <= bound


def test_a_moved_id_boundary_is_a_disocclusion():
    cam, prm, first, second = boundary_frames()
    W = int(cam.width)
    state = accumulate_records(first, None, None, None, None, None, cam, prm)
    got = accumulate_records(second, None, state["records"], None, state["length"], None, cam, prm)
    other = first[:, 7].view(np.uint32) != second[:, 7].view(np.uint32)       # static view: a pixel reprojects onto itself
    assert other.sum() == 3 * (len(first) // W)
    assert (got["length"][other] == 1).all() and same_bits(got["records"][other], second[other])
    assert (got["length"][~other] == 2).all()
    want = (first[~other, 0:3] + F(0.5) * (second[~other, 0:3] - first[~other, 0:3])).astype(F)
    assert same_bits(got["records"][~other, 0:3], want) and same_bits(got["records"][:, 3:], second[:, 3:])


def test_item_motion_and_world_positions():
    """A point of an item that was translated by t between two transform updates lay at world - t before; pixels of other ids do not move."""
    cam, prm, records, _ = static_frames(37, 19, 1)
    world = temporal.world_positions(records[0], cam)
    assert world.shape == (37 * 19, 3) and world.dtype == F and np.isfinite(world).all()
    # the world point lies at the record's depth along the ray from the plane one unit ahead of the eye
    eye = np.asarray(cam.view_inverse)[:3, 3]
    view = (np.concatenate([world, np.ones((len(world), 1))], axis=1) @ np.asarray(cam.view).T)[:, :3]
    dist = np.linalg.norm(world - eye, axis=1)
    assert np.allclose(dist - dist / -view[:, 2], records[0][:, 3], rtol=1e-5)
    ids = records[0][:, 7].view(np.uint32)
    t = np.array([0.25, -0.5, 0.125])
    cur, prev = np.eye(4), np.eye(4)
    cur[:3, 3], prev[:3, 3] = t, 0
    mv = temporal.item_motion(world, ids, [3], [prev], [np.linalg.inv(cur)])
    assert np.allclose(mv[ids == 3], -t, atol=1e-5) and (mv[ids != 3] == 0).all()


# ---- the entry points, without a device -----------------------------------------------------------------------------------------
def test_default_params():
    p = capi.accumulate_default_params()
    assert C.sizeof(capi.rr_accumulate_params) == 100 == p.struct_size
    d = AccumulateParams()
    assert (p.max_history, p.normal_min, p.sigma_depth, p.snap, p.gamma_correction) == (32.0, F(0.9), F(0.05), 1 / 64, 0)
    assert (F(d.max_history), F(d.normal_min), F(d.sigma_depth), F(d.snap)) == (p.max_history, p.normal_min, p.sigma_depth, p.snap)
    assert list(p.prev_world_to_clip) == np.eye(4).reshape(16).tolist() and list(p.prev_eye) == [0, 0, 0]
    assert capi.lib().rr_accumulate_default_params(None) == -1
    q = capi.accumulate_params(AccumulateParams(prev_world_to_clip=np.arange(16, dtype=F).reshape(4, 4), prev_eye=np.array([1, 2, 3], F), max_history=8))
    assert list(q.prev_world_to_clip)[:5] == [0, 4, 8, 12, 1] and list(q.prev_eye) == [1, 2, 3] and q.max_history == 8      # column-major


def test_refusals_without_a_device():
    """Every call below is refused on its arguments alone, before the scene is looked at: the made-up handle is never dereferenced."""
    L = capi.lib()
    W, H = 20, 12
    n = W * H
    cam = capi.rr_camera()
    cam.width, cam.height = W, H
    rec, hist = np.full((n + 4, 8), 0.5, F), np.full((n + 4, 8), 0.5, F)
    halves, hist_h = np.full((n + 4, 2, 8), 0.5, F), np.full((n + 4, 2, 8), 0.5, F)
    hist_l, motion = np.full(n + 4, 1.0, F), np.zeros((n + 4, 3), F)
    out, out_h = np.full((n + 4, 8), 7.0, F), np.full((n + 4, 2, 8), 7.0, F)
    length, rgba = np.full(n + 4, 7.0, F), np.full((n + 4, 4), 0x5a, np.uint8)
    fake = C.c_void_p(0x1000)
    P = lambda a, off=0: C.c_void_p(a.ctypes.data + off)
    good = capi.accumulate_default_params

    for name, dev in (("rr_accumulate_records", False), ("rr_accumulate_records_device", True)):
        fn = getattr(L, name)

        def call(scene=fake, w=W, h=H, prm=None, r=P(rec), hv=P(halves), hi=P(hist), hh=P(hist_h), hl=P(hist_l), mv=P(motion), o=P(out), oh=P(out_h),
                 lo=P(length), rg=P(rgba), null_prm=False, null_cam=False):
            p = prm or good()
            c = capi.rr_camera()
            c.width, c.height = w, h
            args = [scene, None if null_cam else C.byref(c), None if null_prm else C.byref(p), r, hv, hi, hh, hl, mv, o, oh, lo, rg]
            return fn(*(args + [None] if dev else args))

        err = lambda: L.rr_last_error()
        assert call(scene=None) == -1 and b"scene" in err()
        assert call(null_cam=True) == -1 and b"camera" in err()
        assert call(null_prm=True) == -1 and b"params" in err()
        assert call(r=None) == -1 and b"records" in err()
        assert call(o=None) == -1 and b"out is NULL" in err()
        assert call(lo=None) == -1 and b"length_out" in err()
        assert call(w=0) == -1 and call(h=0) == -1 and b"frame size" in err()
        assert call(w=65536, h=1) == -1 and call(w=1, h=65536) == -1 and b"frame size" in err()
        assert call(w=32768, h=16385) == -2 and b"2^30" in err()
        nan, inf = float("nan"), float("inf")
        for fld, values in (("struct_size", (0, 96, 104)), ("max_history", (0.5, 65537.0, nan, inf, -1.0)), ("normal_min", (-1.5, 1.5, nan)),
                            ("sigma_depth", (0.0, -1.0, nan, inf)), ("snap", (-0.1, 0.5, nan, inf))):
            for val in values:
                p = good()
                setattr(p, fld, val)
                assert call(prm=p) == -1, (name, fld, val)
                assert fld.encode() in err(), (name, fld, err())
        # what comes with what
        assert call(hi=None) == -1 and b"history and history_length" in err()
        assert call(hl=None) == -1 and b"history and history_length" in err()
        assert call(hh=None) == -1 and b"history_halves" in err()
        assert call(hv=None, oh=None) == -1 and b"history_halves" in err()            # a half-history without halves
        assert call(hi=None, hl=None) == -1 and b"history_halves" in err()            # a half-history on the first frame
        assert call(oh=None) == -1 and b"halves_out is required" in err()
        assert call(hv=None, hh=None) == -1 and b"halves_out is required" in err()    # halves_out without halves
        # overlaps: only out == records and halves_out == halves, in place, are allowed
        assert call(o=P(rec, 32)) == -1 and b"out overlaps records" in err()
        assert call(o=P(hist)) == -1 and b"out overlaps history" in err()
        assert call(o=P(halves)) == -1 and b"out overlaps halves" in err()
        assert call(oh=P(hist_h)) == -1 and b"halves_out overlaps history_halves" in err()
        assert call(oh=P(halves, 32)) == -1 and b"halves_out overlaps halves" in err()
        assert call(lo=P(hist_l)) == -1 and b"length_out overlaps history_length" in err()
        assert call(lo=P(motion)) == -1 and b"length_out overlaps motion" in err()
        assert call(rg=P(rec)) == -1 and b"rgba8_out overlaps records" in err()
        assert call(lo=P(out, 32 * n - 4)) == -1 and b"out overlaps length_out" in err()
        assert call(oh=P(out)) == -1 and b"out overlaps halves_out" in err()
        assert call(rg=P(length)) == -1 and b"length_out overlaps rgba8_out" in err()
        if dev:   # the alignment rules of the device form
            for kw in (dict(r=P(rec, 8)), dict(hv=P(halves, 4)), dict(hi=P(hist, 8)), dict(hh=P(hist_h, 8)), dict(o=P(out, 8)), dict(oh=P(out_h, 4))):
                assert call(**kw) == -1 and b"16-byte aligned" in err(), kw
            for kw in (dict(hl=P(hist_l, 2)), dict(mv=P(motion, 1)), dict(lo=P(length, 2)), dict(rg=P(rgba, 1))):
                assert call(**kw) == -1 and b"4-byte aligned" in err(), kw
    assert (out == 7.0).all() and (out_h == 7.0).all() and (length == 7.0).all() and (rgba == 0x5a).all()


def test_the_new_entry_points_are_guarded_and_bound():
    src = host_api_source()
    for n in NEW:
        assert re.search(r'^int ' + n + r'\([^{]*\) try \{', src, re.M), f"{n} is not a function-try-block"
        assert f'RR_GUARD_END("{n}")' in src
        assert n in capi.EXPORTS and hasattr(capi.lib(), n) and getattr(capi.lib(), n).argtypes is not None
        assert getattr(C.CDLL(capi.LIB_PATH), n) is not None          # found under its plain name: exported unmangled
    assert "rr_api_temporal.h" in capi.LIB_SOURCES and "rr_temporal.h" in capi.LIB_SOURCES
    mk = open(os.path.join(ROOT, "rustray_amd", "csrc", "Makefile")).read()
    assert "rr_api_temporal.h" in mk and "rr_temporal.h" in mk
    # rr_temporal.h is plain host logic: no system include, no HIP call; what it includes is as plain (rr_denoise.h, rr_pixel_list.h)
    text = open(os.path.join(ROOT, "rustray_amd", "csrc", "rr_temporal.h")).read()
    assert re.findall(r'#include\s+(\S+)', text) == ['"rr_denoise.h"', '"rr_pixel_list.h"']
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    assert not re.search(r"\bhip[A-Z]\w*\s*\(", code)
    for m in ("accumulate_records", "accumulate_records_device"):
        assert hasattr(capi.DeviceScene, m)
    from rustray_amd import renderer
    assert hasattr(renderer, "accumulate_torch") and hasattr(renderer, "render_temporal_torch") and hasattr(renderer, "TemporalState")
    assert hasattr(renderer.Raytracing, "render_temporal")
