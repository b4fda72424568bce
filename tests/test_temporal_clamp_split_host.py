"""rr_accumulate_clamped_split_records without a GPU: the host loop over rustray_amd/csrc/rr_history_clamp.h: history_clamp_split (the
function the kernel applies per lane) under AddressSanitizer + UBSan against the numpy yardstick rustray_amd/temporal.py:
accumulate_clamped_split_records, bit for bit, boxes included; the yardstick against accumulate_clamped_records and
accumulate_split_records (the consequences the header states); the cases have what they promise; and what the entry points refuse
before they touch a device."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from rustray_amd import capi
from rustray_amd.temporal import HistoryClampParams, accumulate_clamped_records, accumulate_split_records, clamp_boxes
from tests import temporal_host_loop
from tests.denoise_cases import F, same_bits
from tests.helpers import ROOT, host_api_source
from tests.temporal_cases import frame_params
from tests.temporal_clamp_split_cases import KINDS, clamp_split_frame, clamp_split_frame_odd, colour_inputs, inputs, own_colour_split_frame

NEW = ("rr_accumulate_clamped_split_records_device", "rr_accumulate_clamped_split_records")
LAYERS = ("records", "length", "halves", "diffuse", "diffuse_halves")


def _yardstick(*a, **kw):
    from rustray_amd.temporal import accumulate_clamped_split_records      # (absent before this call existed: every test here fails then)
    return accumulate_clamped_split_records(*a, **kw)


@pytest.fixture(scope="module")
def host_loop(tmp_path_factory):
    exe = temporal_host_loop.build(tmp_path_factory)

    def run(tmp_path, cam, prm, clamp, args):
        return temporal_host_loop.run(exe, tmp_path, cam, prm, clamp, True, tuple(args))
    return run


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(got, want, what, keys=LAYERS):
    for key in keys:
        if want[key] is None:
            assert got[key] is None, (what, key)
            continue
        g, w = _words(got[key]), _words(want[key])
        assert same_bits(g, w), f"{what}: {int((g != w).sum())} words of {key} differ"


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


# ---- the cases have what they promise ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(37, 19), (130, 70)])
def test_the_clean_case_has_all_four_classes(size):
    """A condition on the inputs, asserted on the yardstick's `clamped` and `diffuse_clamped` at radius 1 and sigma_scale 1: of the pixels
    that kept their history, those whose record layer was moved and those whose diffuse layer was moved, yes or no, make four classes, and
    each holds at least 3 % of them.  (Measured: 0.478 / 0.187 / 0.060 / 0.276 at 37x19 and 0.567 / 0.127 / 0.066 / 0.240 at 130x70 for
    both / colour only / diffuse only / neither.)"""
    case = clamp_split_frame(*size)
    got = _yardstick(*inputs(case, True, True, False), case["cam"], frame_params(case), HistoryClampParams(1, 1.0))
    plain = accumulate_split_records(*inputs(case, True, True, False), case["cam"], frame_params(case))
    kept = plain["taps"]["taken"].any(-1)
    c, d = got["clamped"][kept, 0], got["diffuse_clamped"][kept, 0]
    shares = dict(both=float((c & d).mean()), colour_only=float((c & ~d).mean()), diffuse_only=float((~c & d).mean()), neither=float((~c & ~d).mean()))
    print(size, int(kept.sum()), "kept;", shares, "diffuse halves", got["diffuse_clamped"][kept, 1].mean(), got["diffuse_clamped"][kept, 2].mean())
    assert kept.sum() > 100
    for name, share in shares.items():
        assert share >= 0.03, (size, name, share)
    assert not got["clamped"][~kept].any() and not got["diffuse_clamped"][~kept].any()


@pytest.mark.parametrize("radius,sigma_scale", [(1, 1.0), (2, 1.0), (1, 0.0), (2, 65536.0)])
def test_the_odd_case_has_what_it_promises(radius, sigma_scale):
    """At 130x70.  The diffuse layer holds finite values whose square overflows (the 1e30 channels times u, the 3e38 pairs times u, part of
    the 5e19 channels) and spoiled triples (NaN or inf in a channel, or all three).  EVERY window that holds an overflowing diffuse value
    has no diffuse box in that channel (lo = -inf, hi = +inf).  A spoiled triple is by the header's rule not taken: its window counts one
    point fewer and its box is that of the others -- and a pixel all of whose window is spoiled (here: made so, a 1x1 and a 3x2 frame of
    NaN) has m = 0 and no box in any channel.  At least one kept pixel has a non-finite diffuse of its own; it keeps its current bits, and
    its record layer is accumulate_clamped_records' all the same.  The diffuse box is independent of the colours' finiteness: many
    windows count fewer diffuse triples than colours."""
    W, H = 130, 70
    case = clamp_split_frame_odd(W, H)
    clamp = HistoryClampParams(radius, sigma_scale)
    args = inputs(case, True, True, False)
    got = _yardstick(*args, case["cam"], frame_params(case), clamp)
    kept = got["taps"]["taken"].any(-1)
    dif = case["diffuse"]
    dfin = np.isfinite(dif).all(-1)
    dlo, dhi, _, dm = clamp_boxes(dif, W, H, clamp)
    assert same_bits(dlo, got["diffuse_box"]["lo"]) and same_bits(dhi, got["diffuse_box"]["hi"])
    with np.errstate(all="ignore"):
        overflowing = dfin[:, None] & np.isinf(dif * dif)
    for c in range(3):
        assert overflowing[:, c].sum() >= 20
        holds = _window_holds(overflowing[:, c], W, H, radius)
        assert holds.sum() > 50 and np.isneginf(dlo[holds, c]).all() and np.isposinf(dhi[holds, c]).all(), c
    spoiled = ~dfin & np.isfinite(case["records"][:, 0:3]).all(-1)
    assert spoiled.sum() > 50 and (kept & ~dfin).sum() >= 1
    own = kept & ~dfin
    assert same_bits(got["diffuse"][own], dif[own]) and not got["diffuse_clamped"][own, 0].any()
    # a spoiled point is not counted: m is the number of finite diffuse triples of the window, whatever the colours hold
    count = np.zeros(W * H, np.int64)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            shifted = np.zeros((H, W), bool)
            ys, yq = slice(max(0, -dy), min(H, H - dy)), slice(max(0, dy), min(H, H + dy))
            xs, xq = slice(max(0, -dx), min(W, W - dx)), slice(max(0, dx), min(W, W + dx))
            shifted[ys, xs] = dfin.reshape(H, W)[yq, xq]
            count += shifted.reshape(-1)
    assert np.array_equal(dm, count)
    _, _, _, cm = clamp_boxes(case["records"], W, H, clamp)
    assert (dm < cm).sum() > 50
    boxed = np.isfinite(dlo)
    assert (boxed.any(-1) & _window_holds(spoiled, W, H, radius)).sum() > 50          # (a window with a spoiled point keeps a box from the others)
    for w, h in ((1, 1), (3, 2)):
        lo, hi, _, m = clamp_boxes(np.full((w * h, 3), np.nan, F), w, h, clamp)
        assert (m == 0).all() and np.isneginf(lo).all() and np.isposinf(hi).all()
    # the colour side never sees the diffuse
    colour = accumulate_clamped_records(*colour_inputs(args), case["cam"], frame_params(case), clamp)
    _same(got, colour, "odd colour side", keys=("records", "length", "halves"))


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
        want = _yardstick(*args, case["cam"], prm, clamp)
        got = host_loop(tmp_path, case["cam"], prm, clamp, args)
        what = f"{kind} {size} r={radius} k={sigma_scale} halves={use_halves} motion={use_motion} snap={snap} first={first}"
        _same(got, want, what)
        fin = np.isfinite(case["records"][:, 0:3]).all(-1)
        assert same_bits(got["lo"][fin], want["box"]["lo"][fin]) and same_bits(got["hi"][fin], want["box"]["hi"][fin]), what
        assert same_bits(got["dlo"], want["diffuse_box"]["lo"]) and same_bits(got["dhi"], want["diffuse_box"]["hi"]), what
        if first:
            assert not want["clamped"].any() and not want["diffuse_clamped"].any()


def test_a_frame_whose_diffuse_is_all_spoiled(host_loop, tmp_path):
    """37x19, clean, with every current diffuse triple NaN: no window takes anything, m = 0, no pixel has a diffuse box, and every diffuse
    output keeps its current bits in host loop and yardstick alike, while the colour side goes on as ever."""
    case = dict(clamp_split_frame(37, 19))
    case["diffuse"] = np.full_like(case["diffuse"], np.nan)
    args = inputs(case, True, True, False)
    prm, clamp = frame_params(case), HistoryClampParams(1, 1.0)
    want = _yardstick(*args, case["cam"], prm, clamp)
    got = host_loop(tmp_path, case["cam"], prm, clamp, args)
    _same(got, want, "all spoiled")
    assert np.isneginf(got["dlo"]).all() and np.isposinf(got["dhi"]).all() and same_bits(got["diffuse"], case["diffuse"])
    assert want["clamped"][:, 0].sum() > 20 and not want["diffuse_clamped"].any()          # (the halves have no box to leave either)


# ---- the consequences the header states ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["clean", "odd"])
@pytest.mark.parametrize("size", [(3, 2), (37, 19), (130, 70)])
@pytest.mark.parametrize("radius,sigma_scale", [(1, 1.0), (2, 2.0), (1, 0.0), (2, 65536.0)])
def test_consequences_against_the_two_older_calls(kind, size, radius, sigma_scale):
    case = KINDS[kind](*size)
    prm = frame_params(case)
    clamp = HistoryClampParams(radius, sigma_scale)
    for use_halves, use_motion, first in ((True, True, False), (False, False, False), (True, False, True)):
        args = inputs(case, use_halves, use_motion, first)
        got = _yardstick(*args, case["cam"], prm, clamp)
        colour = accumulate_clamped_records(*colour_inputs(args), case["cam"], prm, clamp)
        split = accumulate_split_records(*args, case["cam"], prm)
        what = f"{kind} {size} {clamp} halves={use_halves} first={first}"
        # the colour side: accumulate_clamped_records' bits in records, halves and length, its flags and its box, whatever the diffuse holds
        _same(got, colour, what, keys=("records", "length", "halves"))
        assert same_bits(got["clamped"], colour["clamped"]) and same_bits(got["box"]["lo"], colour["box"]["lo"]) and same_bits(got["box"]["hi"], colour["box"]["hi"])
        for key in ("x", "y", "weight", "taken", "reprojected"):
            assert same_bits(got["taps"][key], split["taps"][key])
        kept = split["taps"]["taken"].any(-1)
        cl, dcl = got["clamped"], got["diffuse_clamped"]
        assert not cl[~kept].any() and not dcl[~kept].any()
        # 1: every no-history path writes accumulate_split_records' bits in all outputs
        # 3: and so does a pixel in which no layer of either kind leaves its box
        still = ~kept | ~(cl.any(-1) | dcl.any(-1))
        for key in LAYERS:
            if split[key] is not None:
                assert (_words(got[key])[still] == _words(split[key])[still]).all(), (what, key)
        if first:
            assert still.all()
        # 2: a pixel whose record layer was not moved, and in which a diffuse layer L stays inside the diffuse box, has L's split bits
        layers = [(0, got["diffuse"], split["diffuse"])]
        if use_halves:
            layers += [(1 + h, got["diffuse_halves"][:, h], split["diffuse_halves"][:, h]) for h in (0, 1)]
        for index, mine, theirs in layers:
            inside = kept & ~cl[:, 0] & ~dcl[:, index]
            assert (_words(mine)[inside] == _words(theirs)[inside]).all(), (what, index)
            if size == (130, 70) and not first and sigma_scale == 1.0 and kind == "clean":
                moved = kept & dcl[:, index]
                assert inside.sum() > 50 and moved.sum() > 50 and (_words(mine)[moved] != _words(theirs)[moved]).any(-1).mean() > 0.9
        # a moved diffuse layer does not shorten the length: the length is the colour side's, moved or not
        assert same_bits(got["length"], colour["length"])
        # a diffuse layer that keeps its current bits in the split call keeps them here (non-finite current or mean)
        for index, mine, theirs in layers:
            cur = args[2] if index == 0 else args[3][:, index - 1]
            keeps = (_words(theirs) == _words(np.ascontiguousarray(cur))).all(-1) & ~np.isfinite(cur).all(-1)
            assert (_words(mine)[keeps] == _words(np.ascontiguousarray(cur))[keeps]).all()


def test_a_held_diffuse_mean_lies_in_its_box_and_blends_with_the_final_a():
    """130x70 clean, radius 1, sigma_scale 1: where the diffuse layer was moved the output is hd' + a * (cur - hd') with hd' a bound of
    the diffuse box in the moved channels and a = 1 / length_out -- the final a of the colour side, after its length rule."""
    case = clamp_split_frame(130, 70)
    args = inputs(case, False, False, False)
    prm = frame_params(case)
    got = _yardstick(*args, case["cam"], prm, HistoryClampParams(1, 1.0))
    split = accumulate_split_records(*args, case["cam"], prm)
    moved = got["diffuse_clamped"][:, 0]
    shortened = moved & got["clamped"][:, 0] & (got["length"] < split["length"])
    assert moved.sum() > 200 and shortened.sum() > 100
    lo, hi = got["diffuse_box"]["lo"], got["diffuse_box"]["hi"]
    cur = case["diffuse"]
    with np.errstate(all="ignore"):
        a = (F(1) / got["length"]).astype(F)[:, None]
        at_lo, at_hi = (lo + a * (cur - lo)).astype(F), (hi + a * (cur - hi)).astype(F)
    out = got["diffuse"]
    hit = (_words(out) == _words(at_lo)) | (_words(out) == _words(at_hi))
    assert hit[moved].any(-1).all()          # (every moved pixel has a channel that sits on a bound; its other channels may have stayed inside)


def test_own_colours_under_a_wide_box_are_accumulate_split_records():
    """A history that holds the current frame in every layer, colour and diffuse (static view, one tap).  A member of a window of m values
    lies within sqrt(m - 1) standard deviations of its mean -- 2.83 at 3x3, 4.90 at 5x5 --, so at sigma_scale 8 nothing leaves any box
    and every output is accumulate_split_records'."""
    for size in ((37, 19), (130, 70)):
        case, prm = own_colour_split_frame(*size)
        for radius in (1, 2):
            for use_halves in (True, False):
                args = inputs(case, use_halves, False, False)
                got, split = _yardstick(*args, case["cam"], prm, HistoryClampParams(radius, 8.0)), accumulate_split_records(*args, case["cam"], prm)
                assert not got["clamped"].any() and not got["diffuse_clamped"].any() and (split["length"] > 1).mean() > 0.5
                _same(got, split, f"own colours {size} r={radius}")


def test_the_yardstick_refuses_what_the_two_calls_refuse():
    case = clamp_split_frame(37, 19)
    args = inputs(case, True, False, False)
    for radius, k in ((0, 1.0), (3, 1.0), (1, -0.5), (1, float("nan")), (1, float("inf")), (1, 65537.0)):
        with pytest.raises(ValueError):
            _yardstick(*args, case["cam"], frame_params(case), HistoryClampParams(radius, k))
    for at in (2, 3, 5, 6, 7):          # diffuse, diffuse_halves, history_halves, history_diffuse, history_diffuse_halves
        bad = list(args)
        bad[at] = None
        with pytest.raises(ValueError):
            _yardstick(*bad, case["cam"], frame_params(case), HistoryClampParams())


# ---- the entry points, without a device -----------------------------------------------------------------------------------------
def test_refusals_without_a_device():
    """Every call below is refused on its arguments alone, before the scene is looked at: the made-up handle is never dereferenced."""
    L = capi.lib()
    W, H = 20, 12
    n = W * H
    full = lambda shape, v: np.full(shape, v, F)
    rec, hist, halves, hist_h = full((n + 4, 8), 0.5), full((n + 4, 8), 0.5), full((n + 4, 2, 8), 0.5), full((n + 4, 2, 8), 0.5)
    dif, hist_d, dif_h, hist_dh = full((n + 4, 3), 0.25), full((n + 4, 3), 0.25), full((n + 4, 2, 3), 0.25), full((n + 4, 2, 3), 0.25)
    hist_l, motion = full(n + 4, 1.0), np.zeros((n + 4, 3), F)
    out, out_h, out_d, out_dh = full((n + 4, 8), 7.0), full((n + 4, 2, 8), 7.0), full((n + 4, 3), 7.0), full((n + 4, 2, 3), 7.0)
    length, rgba = full(n + 4, 7.0), np.full((n + 4, 4), 0x5a, np.uint8)
    fake = C.c_void_p(0x1000)
    P = lambda a, off=0: C.c_void_p(a.ctypes.data + off)
    good, good_clamp = capi.accumulate_default_params, capi.history_clamp_default_params

    for name, dev in (("rr_accumulate_clamped_split_records", False), ("rr_accumulate_clamped_split_records_device", True)):
        fn = getattr(L, name)

        def call(scene=fake, w=W, h=H, prm=None, clamp=None, r=P(rec), hv=P(halves), d=P(dif), dh=P(dif_h), hi=P(hist), hh=P(hist_h), hd=P(hist_d), hdh=P(hist_dh),
                 hl=P(hist_l), mv=P(motion), o=P(out), oh=P(out_h), od=P(out_d), odh=P(out_dh), lo=P(length), rg=P(rgba), null_prm=False, null_cam=False,
                 null_clamp=False):
            p, k = prm or good(), clamp or good_clamp()
            c = capi.rr_camera()
            c.width, c.height = w, h
            args = [scene, None if null_cam else C.byref(c), None if null_prm else C.byref(p), None if null_clamp else C.byref(k), r, hv, d, dh, hi, hh, hd, hdh, hl, mv,
                    o, oh, od, odh, lo, rg]
            return fn(*(args + [None] if dev else args))

        err = lambda: L.rr_last_error()
        named = lambda text: text in err() and name.encode() + b":" in err()
        assert call(scene=None) == -1 and named(b"scene")
        assert call(null_cam=True) == -1 and named(b"camera")
        assert call(null_prm=True) == -1 and named(b"params")
        assert call(null_clamp=True) == -1 and named(b"clamp is NULL")
        assert call(r=None) == -1 and named(b"records")
        assert call(o=None) == -1 and named(b"out is NULL")
        assert call(lo=None) == -1 and named(b"length_out")
        assert call(d=None) == -1 and named(b"diffuse is NULL")
        assert call(od=None) == -1 and named(b"diffuse_out is NULL")
        assert call(w=0) == -1 and call(h=0) == -1 and named(b"frame size")
        assert call(w=65536, h=1) == -1 and call(w=1, h=65536) == -1 and named(b"frame size")
        assert call(w=32768, h=16385) == -2 and named(b"2^30")
        nan, inf = float("nan"), float("inf")
        for fld, values in (("struct_size", (0, 96, 104)), ("max_history", (0.5, 65537.0, nan, inf, -1.0)), ("normal_min", (-1.5, 1.5, nan)),
                            ("sigma_depth", (0.0, -1.0, nan, inf)), ("snap", (-0.1, 0.5, nan, inf))):
            for val in values:
                p = good()
                setattr(p, fld, val)
                assert call(prm=p) == -1 and named(fld.encode()), (name, fld, val, err())
        for fld, values in (("struct_size", (0, 8, 16)), ("radius", (0, 3, 0xffffffff)), ("sigma_scale", (nan, inf, -inf, -0.5, 65537.0))):
            for val in values:
                k = good_clamp()
                setattr(k, fld, val)
                assert call(clamp=k) == -1 and named(b"clamp->" + fld.encode()), (name, fld, val, err())
        # what comes with what: the rules of rr_accumulate_records and of rr_accumulate_split_records
        assert call(hi=None) == -1 and named(b"history and history_length")
        assert call(hl=None) == -1 and named(b"history and history_length")
        assert call(hh=None) == -1 and named(b"history_halves")
        assert call(oh=None) == -1 and named(b"halves_out is required")
        assert call(dh=None) == -1 and named(b"diffuse_halves is required")
        assert call(odh=None) == -1 and named(b"diffuse_halves_out is required")
        assert call(hd=None) == -1 and named(b"history_diffuse is required")
        assert call(hdh=None) == -1 and named(b"history_diffuse_halves is required")
        # overlaps: out may not lie on records and diffuse_out not on diffuse at all, the in-place pointers included, refused by name with the
        # reason; the halves in place stay allowed (such a call would go on to the made-up handle: only shifted halves are tried)
        assert call(o=P(rec)) == -1 and named(b"out overlaps records") and b"windows read" in err()
        assert call(o=P(rec, 32)) == -1 and named(b"out overlaps records")
        assert call(od=P(dif)) == -1 and named(b"diffuse_out overlaps diffuse ") and b"windows read" in err()
        assert call(od=P(dif, 12)) == -1 and named(b"diffuse_out overlaps diffuse ")
        assert call(o=P(hist)) == -1 and named(b"out overlaps history")
        assert call(od=P(hist_d)) == -1 and named(b"diffuse_out overlaps history_diffuse")
        assert call(oh=P(halves, 32)) == -1 and named(b"halves_out overlaps halves")
        assert call(odh=P(dif_h, 12)) == -1 and named(b"diffuse_halves_out overlaps diffuse_halves")
        assert call(oh=P(hist_h)) == -1 and named(b"halves_out overlaps history_halves")
        assert call(odh=P(hist_dh)) == -1 and named(b"diffuse_halves_out overlaps history_diffuse_halves")
        assert call(lo=P(hist_l)) == -1 and named(b"length_out overlaps history_length")
        assert call(rg=P(motion)) == -1 and named(b"rgba8_out overlaps motion")
        assert call(oh=P(out)) == -1 and named(b"out overlaps halves_out")
        assert call(odh=P(out_d)) == -1 and named(b"diffuse_out overlaps diffuse_halves_out")
        assert call(lo=P(out_h)) == -1 and named(b"halves_out overlaps length_out")
        if dev:   # the alignment rules of the device form
            for kw in (dict(r=P(rec, 8)), dict(hv=P(halves, 4)), dict(hi=P(hist, 8)), dict(hh=P(hist_h, 8)), dict(o=P(out, 8)), dict(oh=P(out_h, 4))):
                assert call(**kw) == -1 and named(b"16-byte aligned"), kw
            for kw in (dict(hl=P(hist_l, 2)), dict(mv=P(motion, 1)), dict(lo=P(length, 2)), dict(rg=P(rgba, 1)), dict(d=P(dif, 2)), dict(dh=P(dif_h, 1)), dict(hd=P(hist_d, 2)),
                       dict(hdh=P(hist_dh, 3)), dict(od=P(out_d, 2)), dict(odh=P(out_dh, 1))):
                assert call(**kw) == -1 and named(b"4-byte aligned"), kw
    for a in (out, out_h, out_d, out_dh, length):
        assert (a == 7.0).all()
    assert (rgba == 0x5a).all()


def test_the_new_entry_points_are_guarded_and_bound():
    src = host_api_source()
    for n in NEW:
        assert re.search(r'^int ' + n + r'\([^{]*\) try \{', src, re.M), f"{n} is not a function-try-block"
        assert f'RR_GUARD_END("{n}")' in src
        assert n in capi.EXPORTS and hasattr(capi.lib(), n) and getattr(capi.lib(), n).argtypes is not None
        assert getattr(C.CDLL(capi.LIB_PATH), n) is not None          # found under its plain name: exported unmangled
    assert len(capi.lib().rr_accumulate_clamped_split_records.argtypes) == 20 and len(capi.lib().rr_accumulate_clamped_split_records_device.argtypes) == 21
    header = open(os.path.join(ROOT, "include", "rustray_hip.h")).read()
    for n in NEW:
        assert re.search(r'^int ' + n + r'\(', header, re.M)
    lacks = header[:header.index("#define RR_ABI_VERSION")]
    assert "rr_accumulate_clamped_split_records and rr_accumulate_clamped_split_records_device" in lacks
    # no new struct; the staging pool keeps its 16 slots, which the host form's sixteen arrays fill
    assert len(re.findall(r"^typedef struct rr_history_clamp_params", header, re.M)) == 1 and "clamped_split" not in "".join(re.findall(r"typedef struct (\w+)", header))
    handle = open(os.path.join(ROOT, "rustray_amd", "csrc", "rr_api_handle.h")).read()
    assert re.search(r"struct RecordStage \{\s*DevBuf buf\[16\];", handle)
    for entry in ("int rr_accumulate_clamped_split_records(", "int rr_accumulate_split_records("):
        body = src[src.index(entry):]
        body = re.sub(r"\s+", " ", body[:body.index("RR_GUARD_END")])
        assert "accumulate_call(" in body and ("AccumulateIo{records, halves, diffuse, diffuse_halves, history, history_halves, history_diffuse, history_diffuse_halves, "
                                               "history_length, motion, out, halves_out, diffuse_out, diffuse_halves_out, length_out, rgba8_out}") in body
    call = src[src.index("static int accumulate_call("):]
    call = call[:call.index("\n}\n")]
    assert re.search(r"StageArg args\[ACC_ROWS\]", call) and "staged_host_call(s->record_stage.buf, args," in call and "enum { ACC_ROWS = 16 }" in src
    # rr_history_clamp.h stays plain host logic over rr_temporal.h and has the diffuse side next to history_clamp
    csrc = os.path.join(ROOT, "rustray_amd", "csrc")
    clamp_h = open(os.path.join(csrc, "rr_history_clamp.h")).read()
    assert re.findall(r'#include\s+(\S+)', clamp_h) == ['"rr_temporal.h"'] and "history_clamp_split(" in clamp_h
    assert "k_accumulate_clamped_split_records" in open(os.path.join(csrc, "rr_kernels.hip")).read()
    for m in ("accumulate_clamped_split", "accumulate_clamped_split_device"):
        assert hasattr(capi.DeviceScene, m)
    from rustray_amd import renderer
    assert "in_place" not in inspect.signature(renderer.accumulate_clamped_split_torch).parameters
    for f in (renderer.render_temporal_split_clamped_torch, renderer.Raytracing.render_temporal_split_clamped):
        assert inspect.signature(f).parameters["clamp"].default is True
    assert "track_items" in inspect.signature(renderer.Raytracing.render_temporal_split_clamped).parameters
    for f in (renderer.render_temporal_split_torch, renderer.Raytracing.render_temporal_split):
        assert inspect.signature(f).parameters["clamp"].default is None
    with pytest.raises(ValueError, match="render_temporal_split_clamped"):
        renderer._no_split_clamp(True)
    host = open(os.path.join(ROOT, "include", "rustray_host.hpp")).read()
    assert "accumulate_clamped_split(" in host and "accumulate_clamped_split_device(" in host
    assert "rh_accumulate_clamped_split" in open(os.path.join(csrc, "host_shim.cpp")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in NEW:
        assert "pub fn " + n + "(" in doc
