"""rr_accumulate_clamped_records without a GPU: the host loop over rustray_amd/csrc/rr_history_clamp.h (the functions the kernel applies per
lane) under AddressSanitizer + UBSan against the numpy yardstick rustray_amd/temporal.py: accumulate_clamped_records, bit for bit; the
yardstick against accumulate_records (the properties the header states); the two older yardsticks against digests of what they gave
before the tap walk got its hook; and what the entry points refuse before they touch a device."""
import ctypes as C
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

from rustray_amd import capi
from rustray_amd.temporal import EPS, HistoryClampParams, accumulate_clamped_records, accumulate_records, accumulate_split_records, clamp_boxes
from tests import temporal_host_loop
from tests.denoise_cases import F, same_bits
from tests.helpers import ROOT, host_api_source
from tests.temporal_cases import frame_params, temporal_frame
from tests.temporal_clamp_cases import KINDS, clamp_frame, clamp_frame_odd, inputs, own_colour_frame
from tests.temporal_split_cases import split_frame_odd

NEW = ("rr_accumulate_clamped_records_device", "rr_accumulate_clamped_records")


@pytest.fixture(scope="module")
def host_loop(tmp_path_factory):
    exe = temporal_host_loop.build(tmp_path_factory)

    def run(tmp_path, cam, prm, clamp, records, halves, history, history_halves, history_length, motion):
        return temporal_host_loop.run(exe, tmp_path, cam, prm, clamp, False, (records, halves, history, history_halves, history_length, motion))
    return run


def _same(got, want, what, keys=("records", "length", "halves")):
    for key in keys:
        if want[key] is None:
            assert got[key] is None
            continue
        g, w = np.ascontiguousarray(got[key]).view(np.uint32), np.ascontiguousarray(want[key]).view(np.uint32)
        assert same_bits(g, w), f"{what}: {int((g != w).sum())} words of {key} differ"


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the cases have what they promise ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("size", [(33, 9), (37, 19), (130, 70)])
def test_the_case_has_what_it_promises(size, radius):
    """A condition on the inputs, asserted on the yardstick's `clamped`: of the pixels that kept their history, at sigma_scale 1 at least
    5 % are clamped in the record layer and at least 5 % are not; at sigma_scale 2 at least 2 % are clamped."""
    case = clamp_frame(*size)
    for k, low, high in ((1.0, 0.05, 0.95), (2.0, 0.02, 1.0)):
        got = accumulate_clamped_records(*inputs(case, True, True, False), case["cam"], frame_params(case), HistoryClampParams(radius, k))
        plain = accumulate_records(*inputs(case, True, True, False), case["cam"], frame_params(case))
        kept = plain["taps"]["taken"].any(-1)
        share = float(got["clamped"][kept, 0].mean())
        print(size, radius, k, f"{int(kept.sum())} kept, share clamped {share:.3f}, halves {got['clamped'][kept, 1].mean():.3f} {got['clamped'][kept, 2].mean():.3f}")
        assert kept.sum() > 20 and low <= share <= high, (size, radius, k, share)
        assert not got["clamped"][~kept].any()


def _window_holds(mask, W, H, r):
    """(n,) bool: the (2r + 1)^2 window of the pixel holds a pixel of `mask` (n,)"""
    m = mask.reshape(H, W)
    out = np.zeros((H, W), bool)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            ys, yq = slice(max(0, -dy), min(H, H - dy)), slice(max(0, dy), min(H, H + dy))
            xs, xq = slice(max(0, -dx), min(W, W - dx)), slice(max(0, dx), min(W, W + dx))
            out[ys, xs] |= m[yq, xq]
    return out.reshape(-1)


@pytest.mark.parametrize("radius,sigma_scale", [(1, 1.0), (2, 1.0), (1, 0.0), (2, 65536.0)])
def test_the_odd_case_has_what_it_promises(radius, sigma_scale):
    """At 130x70.  Some kept pixels have a box that is a point (e = 0: the flat patch).  Each kind of huge colour -- 1e30 (s2 / m and
    mean * mean both overflow: v = inf - inf), 5e19 (only s2 / m overflows: v = inf) and the 3e38 pairs (s1 overflows) -- is there, the
    overflow it stands for really happens in binary32, and EVERY window that holds one has no box in that channel (lo = -inf, hi = +inf):
    no box anywhere is a point far from the colours around it.  Of the kept pixels at least 20 per kind have such a window; below -inf and
    above +inf there is nothing, so no history mean is moved in such a channel, and a kept pixel none of whose other channels leaves its
    box has accumulate_records' bits."""
    W, H = 130, 70
    case = clamp_frame_odd(W, H)
    args = inputs(case, True, True, False)
    plain = accumulate_records(*args, case["cam"], frame_params(case))
    got = accumulate_clamped_records(*args, case["cam"], frame_params(case), HistoryClampParams(radius, sigma_scale))
    kept = plain["taps"]["taken"].any(-1)
    lo, hi, e, m = clamp_boxes(case["records"], W, H, HistoryClampParams(radius, sigma_scale))
    col = case["records"][:, 0:3]
    fin = np.isfinite(col).all(-1)
    if sigma_scale == 1.0:
        assert (kept & (e == 0).all(-1)).sum() >= (5 if radius == 1 else 1)
    with np.errstate(all="ignore"):
        nine = F(9)
        assert np.isinf(F(1e30) * F(1e30)) and np.isinf((F(1e30) / nine) * (F(1e30) / nine))
        assert np.isinf(F(5e19) * F(5e19)) and np.isfinite((F(5e19) / nine) * (F(5e19) / nine)) and np.isfinite(F(5e19) * F(25))
        assert np.isinf(F(3e38) + F(3e38))
    for value in (F(1e30), F(5e19), F(3e38)):
        for c in range(3):
            holds = _window_holds(fin & (col[:, c] == value), W, H, radius) & fin
            if value != F(3e38):
                assert holds.sum() > 50, (value, c)
            assert np.isneginf(lo[holds, c]).all() and np.isposinf(hi[holds, c]).all(), (value, c)
        holds_any = _window_holds(fin & (col == value).any(-1), W, H, radius) & kept
        assert holds_any.sum() >= 20, (value, int(holds_any.sum()))
        still = holds_any & ~got["clamped"].any(-1)
        assert (_words(got["records"])[still] == _words(plain["records"])[still]).all() and (_words(got["length"])[still] == _words(plain["length"])[still]).all()
        if sigma_scale == 65536.0:
            assert still.sum() >= 20
    # every box that exists lies among the colours of its window: no bound beyond the largest finite-boxed colour around
    boxed = np.isfinite(lo) & fin[:, None]
    assert (np.abs(lo[boxed]) < 1.9e19).all() and (np.abs(hi[boxed]) < 1.9e19 * (1 + sigma_scale * 5)).all()
    _, _, _, m_clean = clamp_boxes(clamp_frame(W, H)["records"], W, H, HistoryClampParams(1, 1.0))
    fin_clean = np.isfinite(clamp_frame(W, H)["records"][:, 0:3]).all(-1)
    assert (m_clean[fin_clean] < 9).sum() > 100 and (m_clean[fin_clean] >= 1).all()


# ---- the host loop against the yardstick --------------------------------------------------------------------------------------------
CONFIGS = [(True, True, 1 / 64, False), (True, False, 0.0, False), (False, True, 0.0, False), (False, False, 1 / 64, False), (True, False, 1 / 64, True),
           (False, True, 1 / 64, True)]
CLAMPS = [(1, 0.0), (1, 0.5), (1, 1.0), (2, 1.0), (2, 2.0), (1, 65536.0), (2, 0.0)]


@pytest.mark.parametrize("kind", ["clean", "odd"])
@pytest.mark.parametrize("size", [(1, 1), (3, 2), (37, 19), (130, 70)])
@pytest.mark.parametrize("radius,sigma_scale", CLAMPS)
def test_host_loop_equals_the_yardstick(host_loop, tmp_path, kind, size, radius, sigma_scale):
    case = KINDS[kind](*size)
    clamp = HistoryClampParams(radius, sigma_scale)
    for use_halves, use_motion, snap, first in CONFIGS:
        prm = frame_params(case, snap=snap)
        args = inputs(case, use_halves, use_motion, first)
        want = accumulate_clamped_records(*args, case["cam"], prm, clamp)
        got = host_loop(tmp_path, case["cam"], prm, clamp, *args)
        what = f"{kind} {size} r={radius} k={sigma_scale} halves={use_halves} motion={use_motion} snap={snap} first={first}"
        _same(got, want, what)
        fin = np.isfinite(case["records"][:, 0:3]).all(-1)
        assert same_bits(got["lo"][fin], want["box"]["lo"][fin]) and same_bits(got["hi"][fin], want["box"]["hi"][fin]), what
        if first:
            assert not want["clamped"].any()


# ---- the properties the header states, against accumulate_records ------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["clean", "odd"])
@pytest.mark.parametrize("size", [(3, 2), (37, 19), (130, 70)])
@pytest.mark.parametrize("radius,sigma_scale", [(1, 1.0), (2, 2.0), (1, 0.0), (2, 65536.0)])
def test_properties_against_accumulate_records(kind, size, radius, sigma_scale):
    case = KINDS[kind](*size)
    prm = frame_params(case)
    clamp = HistoryClampParams(radius, sigma_scale)
    for use_halves, use_motion, first in ((True, True, False), (False, False, False), (True, False, True)):
        args = inputs(case, use_halves, use_motion, first)
        got, plain = accumulate_clamped_records(*args, case["cam"], prm, clamp), accumulate_records(*args, case["cam"], prm)
        kept = plain["taps"]["taken"].any(-1)
        cl = got["clamped"]
        # every no-history path writes accumulate_records' bits, and so does a pixel in which no layer leaves its box
        still = ~kept | ~cl.any(-1)
        assert (_words(got["records"])[still] == _words(plain["records"])[still]).all()
        assert (_words(got["length"])[still] == _words(plain["length"])[still]).all()
        if use_halves:
            assert (_words(got["halves"])[still] == _words(plain["halves"])[still]).all()
        # a pixel in which only a half leaves the box differs in that half alone
        if use_halves:
            for h in (0, 1):
                only = kept & ~cl[:, 0] & cl[:, 1 + h] & ~cl[:, 2 - h]
                assert (_words(got["records"])[only] == _words(plain["records"])[only]).all() and (_words(got["length"])[only] == _words(plain["length"])[only]).all()
                assert (_words(got["halves"])[only, 1 - h] == _words(plain["halves"])[only, 1 - h]).all()
        # depth, normal and id are the current record's; a clamped record layer never lengthens the history
        assert same_bits(got["records"][:, 3:8], case["records"][:, 3:8])
        if use_halves:
            assert same_bits(got["halves"][:, :, 3:8], case["halves"][:, :, 3:8])
        assert (got["length"] <= plain["length"]).all() and (got["length"][cl[:, 0]] >= 1).all()
        if size == (130, 70) and not first and sigma_scale <= 2.0:
            assert (got["length"][cl[:, 0]] < plain["length"][cl[:, 0]]).any()
        for key in ("x", "y", "weight", "taken", "reprojected"):
            assert same_bits(got["taps"][key], plain["taps"][key])


def test_sigma_scale_zero_pulls_the_history_onto_the_window_mean():
    """With k = 0 and a boxed channel lo = hi = mean: a kept pixel whose history mean is not the window's mean is moved, its keep is
    1 / (1 + |h - mean| / EPS), and the output is mean + a * (cur - mean)."""
    case = clamp_frame(37, 19)
    prm = frame_params(case)
    got = accumulate_clamped_records(*inputs(case, False, False, False), case["cam"], prm, HistoryClampParams(1, 0.0))
    assert same_bits(got["box"]["lo"], got["box"]["hi"])
    moved = got["clamped"][:, 0]
    assert moved.sum() > 50
    mean = got["box"]["lo"]
    cur = case["records"][:, 0:3]
    with np.errstate(all="ignore"):
        a = (F(1) / got["length"]).astype(F)[:, None]
        want = (mean + a * (cur - mean)).astype(F)
    every = moved & np.isfinite(mean).all(-1)
    plain = accumulate_records(*inputs(case, False, False, False), case["cam"], prm)
    # (a channel that sat on the mean already keeps its own bits, which are the mean's)
    assert same_bits(got["records"][every, 0:3], want[every])
    assert (got["length"][every] < F(1.001)).mean() > 0.9 and float(EPS) == 2.0 ** -20 and (plain["length"][every] > 1).all()


def test_own_colours_under_a_wide_box_are_accumulate_records():
    """A history that holds the current frame's own colours (static view, one tap: h is the pixel's colour).  A member of a window of m
    values lies within sqrt(m - 1) standard deviations of its mean -- 2.83 at 3x3, 4.90 at 5x5 --, so at sigma_scale 8 nothing leaves
    any box and every output is accumulate_records'."""
    for size in ((37, 19), (130, 70)):
        case, prm = own_colour_frame(*size)
        for radius in (1, 2):
            for use_halves in (True, False):
                args = inputs(case, use_halves, False, False)
                got, plain = accumulate_clamped_records(*args, case["cam"], prm, HistoryClampParams(radius, 8.0)), accumulate_records(*args, case["cam"], prm)
                assert not got["clamped"][:, 0].any() and (plain["length"] > 1).mean() > 0.5
                _same(got, plain, f"own colours {size} r={radius}", keys=("records", "length"))


def test_a_pixel_in_which_only_a_half_leaves_the_box_differs_in_that_half_alone():
    """own_colour_frame at sigma_scale 8 (nothing leaves a box) with the half-0 history of every seventh pixel pushed far out: those pixels
    -- where they kept their history -- differ from accumulate_records in half 0 alone, and nothing else differs anywhere."""
    case, prm = own_colour_frame(37, 19)
    hist_h = case["history_halves"].copy()
    pushed = np.zeros(37 * 19, bool)
    pushed[::7] = True
    pushed &= np.isfinite(hist_h[:, 0, 0:3]).all(-1)
    hist_h[pushed, 0, 0:3] += F(1000)
    args = (case["records"], case["halves"], case["history"], hist_h, case["history_length"], None)
    got, plain = accumulate_clamped_records(*args, case["cam"], prm, HistoryClampParams(1, 8.0)), accumulate_records(*args, case["cam"], prm)
    kept = plain["taps"]["taken"].any(-1)
    only = got["clamped"][:, 1] & ~got["clamped"][:, 0] & ~got["clamped"][:, 2]
    assert only.sum() > 20 and (only <= (pushed & kept)).all() and not got["clamped"][:, [0, 2]].any()
    assert same_bits(got["records"], plain["records"]) and same_bits(got["length"], plain["length"]) and same_bits(got["halves"][:, 1], plain["halves"][:, 1])
    differs = (_words(got["halves"][:, 0]) != _words(plain["halves"][:, 0])).any(-1)
    assert (differs <= only).all() and differs.sum() > 20


# ---- the older yardsticks keep their bits --------------------------------------------------------------------------------------------
def _digest(res, keys):
    h = hashlib.sha256()
    for k in keys:
        h.update(np.ascontiguousarray(res[k]).tobytes())
    for k in ("x", "y", "weight", "taken", "reprojected"):
        h.update(np.ascontiguousarray(res["taps"][k]).tobytes())
    return h.hexdigest()[:16]


RECORDS_DIGEST = "8c1b103b671b8b31"
SPLIT_DIGEST = "a49b17ff92e0b421"


def test_accumulate_records_and_accumulate_split_records_give_the_bits_they_gave():
    """Digests taken before _accumulate got its hook: temporal_frame(37, 19) with halves and motion, and split_frame_odd(37, 19)."""
    case = temporal_frame(37, 19)
    got = accumulate_records(*inputs(case, True, True, False), case["cam"], frame_params(case))
    assert _digest(got, ("records", "length", "halves")) == RECORDS_DIGEST
    case = split_frame_odd(37, 19)
    keys = ("records", "halves", "diffuse", "diffuse_halves", "history", "history_halves", "history_diffuse", "history_diffuse_halves", "history_length", "motion")
    got = accumulate_split_records(*(case[k] for k in keys), case["cam"], frame_params(case))
    assert _digest(got, ("records", "length", "halves", "diffuse", "diffuse_halves")) == SPLIT_DIGEST


def test_the_yardstick_refuses_bad_clamps():
    case = clamp_frame(37, 19)
    args = inputs(case, True, False, False)
    for radius, k in ((0, 1.0), (3, 1.0), (1, -0.5), (1, float("nan")), (1, float("inf")), (1, 65537.0)):
        with pytest.raises(ValueError):
            accumulate_clamped_records(*args, case["cam"], frame_params(case), HistoryClampParams(radius, k))
    bad = list(args)
    bad[3] = None
    with pytest.raises(ValueError):
        accumulate_clamped_records(*bad, case["cam"], frame_params(case), HistoryClampParams())
    d = capi.history_clamp_default_params()
    assert (HistoryClampParams().radius, HistoryClampParams().sigma_scale) == (d.radius, d.sigma_scale) and d.struct_size == 12


# ---- the entry points, without a device -----------------------------------------------------------------------------------------
def test_refusals_without_a_device():
    """Every call below is refused on its arguments alone, before the scene is looked at: the made-up handle is never dereferenced."""
    L = capi.lib()
    W, H = 20, 12
    n = W * H
    rec, hist = np.full((n + 4, 8), 0.5, F), np.full((n + 4, 8), 0.5, F)
    halves, hist_h = np.full((n + 4, 2, 8), 0.5, F), np.full((n + 4, 2, 8), 0.5, F)
    hist_l, motion = np.full(n + 4, 1.0, F), np.zeros((n + 4, 3), F)
    out, out_h = np.full((n + 4, 8), 7.0, F), np.full((n + 4, 2, 8), 7.0, F)
    length, rgba = np.full(n + 4, 7.0, F), np.full((n + 4, 4), 0x5a, np.uint8)
    fake = C.c_void_p(0x1000)
    P = lambda a, off=0: C.c_void_p(a.ctypes.data + off)
    good, good_clamp = capi.accumulate_default_params, capi.history_clamp_default_params

    for name, dev in (("rr_accumulate_clamped_records", False), ("rr_accumulate_clamped_records_device", True)):
        fn = getattr(L, name)

        def call(scene=fake, w=W, h=H, prm=None, clamp=None, r=P(rec), hv=P(halves), hi=P(hist), hh=P(hist_h), hl=P(hist_l), mv=P(motion), o=P(out), oh=P(out_h),
                 lo=P(length), rg=P(rgba), null_prm=False, null_cam=False, null_clamp=False):
            p, k = prm or good(), clamp or good_clamp()
            c = capi.rr_camera()
            c.width, c.height = w, h
            args = [scene, None if null_cam else C.byref(c), None if null_prm else C.byref(p), None if null_clamp else C.byref(k), r, hv, hi, hh, hl, mv, o, oh, lo, rg]
            return fn(*(args + [None] if dev else args))

        err = lambda: L.rr_last_error()
        assert call(scene=None) == -1 and b"scene" in err()
        assert call(null_cam=True) == -1 and b"camera" in err()
        assert call(null_prm=True) == -1 and b"params" in err()
        assert call(null_clamp=True) == -1 and b"clamp is NULL" in err() and name.encode() in err()
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
                assert fld.encode() in err() and name.encode() in err(), (name, fld, err())
        for fld, values in (("struct_size", (0, 8, 16)), ("radius", (0, 3, 0xffffffff)), ("sigma_scale", (nan, inf, -inf, -0.5, 65537.0))):
            for val in values:
                k = good_clamp()
                setattr(k, fld, val)
                assert call(clamp=k) == -1, (name, fld, val)
                assert b"clamp->" + fld.encode() in err() and name.encode() in err(), (name, fld, err())
        # what comes with what: the rules of rr_accumulate_records
        assert call(hi=None) == -1 and b"history and history_length" in err()
        assert call(hl=None) == -1 and b"history and history_length" in err()
        assert call(hh=None) == -1 and b"history_halves" in err()
        assert call(oh=None) == -1 and b"halves_out is required" in err()
        # overlaps: out may not lie on records at all, the in-place pointer included; halves in place stays allowed (the call then goes on
        # to the made-up handle, which this test must not reach: only shifted halves are tried)
        assert call(o=P(rec)) == -1 and b"out overlaps records" in err() and b"window reads" in err()
        assert call(o=P(rec, 32)) == -1 and b"out overlaps records" in err()
        assert call(o=P(hist)) == -1 and b"out overlaps history" in err()
        assert call(oh=P(halves, 32)) == -1 and b"halves_out overlaps halves" in err()
        assert call(oh=P(hist_h)) == -1 and b"halves_out overlaps history_halves" in err()
        assert call(lo=P(hist_l)) == -1 and b"length_out overlaps history_length" in err()
        assert call(rg=P(motion)) == -1 and b"rgba8_out overlaps motion" in err()
        assert call(oh=P(out)) == -1 and b"out overlaps halves_out" in err()
        assert call(lo=P(out_h)) == -1 and b"halves_out overlaps length_out" in err()
        if dev:   # the alignment rules of the device form
            for kw in (dict(r=P(rec, 8)), dict(hv=P(halves, 4)), dict(hi=P(hist, 8)), dict(hh=P(hist_h, 8)), dict(o=P(out, 8)), dict(oh=P(out_h, 4))):
                assert call(**kw) == -1 and b"16-byte aligned" in err(), kw
            for kw in (dict(hl=P(hist_l, 2)), dict(mv=P(motion, 1)), dict(lo=P(length, 2)), dict(rg=P(rgba, 1))):
                assert call(**kw) == -1 and b"4-byte aligned" in err(), kw
    for a in (out, out_h, length):
        assert (a == 7.0).all()
    assert (rgba == 0x5a).all()
    assert L.rr_history_clamp_default_params(None) == -1 and b"rr_history_clamp_default_params" in L.rr_last_error()


def test_the_new_entry_points_are_guarded_and_bound():
    src = host_api_source()
    for n in NEW + ("rr_history_clamp_default_params",):
        assert re.search(r'^int ' + n + r'\([^{]*\) try \{', src, re.M), f"{n} is not a function-try-block"
        assert f'RR_GUARD_END("{n}")' in src
        assert n in capi.EXPORTS and hasattr(capi.lib(), n) and getattr(capi.lib(), n).argtypes is not None
        assert getattr(C.CDLL(capi.LIB_PATH), n) is not None          # found under its plain name: exported unmangled
    assert len(capi.lib().rr_accumulate_clamped_records.argtypes) == 14 and len(capi.lib().rr_accumulate_clamped_records_device.argtypes) == 15
    header = open(os.path.join(ROOT, "include", "rustray_hip.h")).read()
    for n in NEW + ("rr_history_clamp_default_params",):
        assert re.search(r'^int ' + n + r'\(', header, re.M)
    # the staging pool keeps its slots; the host form stages ten arrays
    handle = open(os.path.join(ROOT, "rustray_amd", "csrc", "rr_api_handle.h")).read()
    assert re.search(r"struct RecordStage \{\s*DevBuf buf\[16\];", handle)
    body = src[src.index("int rr_accumulate_clamped_records("):]
    body = re.sub(r"\s+", " ", body[:body.index("RR_GUARD_END")])
    assert "accumulate_call(" in body and ("AccumulateIo{records, halves, nullptr, nullptr, history, history_halves, nullptr, nullptr, history_length, motion, out, "
                                           "halves_out, nullptr, nullptr, length_out, rgba8_out}") in body      # ten arrays: the six diffuse rows are left out
    call = src[src.index("static int accumulate_call("):]
    call = call[:call.index("\n}\n")]
    assert re.search(r"StageArg args\[ACC_ROWS\]", call) and "staged_host_call(s->record_stage.buf, args," in call and "enum { ACC_ROWS = 16 }" in src
    # rr_history_clamp.h is plain host logic over rr_temporal.h, which keeps its own include list; the Makefile and LIB_SOURCES know it
    csrc = os.path.join(ROOT, "rustray_amd", "csrc")
    assert re.findall(r'#include\s+(\S+)', open(os.path.join(csrc, "rr_history_clamp.h")).read()) == ['"rr_temporal.h"']
    assert re.findall(r'#include\s+(\S+)', open(os.path.join(csrc, "rr_temporal.h")).read()) == ['"rr_denoise.h"', '"rr_pixel_list.h"']
    assert "rr_history_clamp.h" in capi.LIB_SOURCES and "rr_history_clamp.h" in open(os.path.join(csrc, "Makefile")).read()
    for m in ("accumulate_clamped", "accumulate_clamped_device"):
        assert hasattr(capi.DeviceScene, m)
    from rustray_amd import renderer
    import inspect
    assert hasattr(renderer, "accumulate_clamped_torch")
    for f in (renderer.render_temporal_torch, renderer.Raytracing.render_temporal, renderer.render_temporal_split_torch, renderer.Raytracing.render_temporal_split):
        assert inspect.signature(f).parameters["clamp"].default is None
    host = open(os.path.join(ROOT, "include", "rustray_host.hpp")).read()
    assert "struct HistoryClamp" in host and "accumulate_clamped(" in host and "accumulate_clamped_device(" in host
    assert "rh_accumulate_clamped" in open(os.path.join(csrc, "host_shim.cpp")).read()


def test_struct_in_a_c99_host(tmp_path):
    exe = str(tmp_path / "history_clamp_c99")
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "history_clamp_c99.c"),
                           "-L" + libdir, "-lrustray_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "history clamp c99 OK" in out.stdout, out.stdout + out.stderr
    assert C.sizeof(capi.rr_history_clamp_params) == 12
    assert [(f, getattr(capi.rr_history_clamp_params, f).offset) for f, _ in capi.rr_history_clamp_params._fields_] == [("struct_size", 0), ("radius", 4), ("sigma_scale", 8)]
