"""rr_accumulate_split_records without a GPU: the host loop over rustray_amd/csrc/rr_temporal.h (the functions the kernel applies per
lane) under AddressSanitizer + UBSan against the numpy yardstick rustray_amd/temporal.py: accumulate_split_records, bit for bit; the
yardstick against accumulate_records (the records ignore the diffuse, and a diffuse layer is what accumulate_records makes of it as a
colour); a static view; and what the entry points refuse before they touch a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from rustray_amd import capi
from rustray_amd.temporal import accumulate_records, accumulate_split_records
from tests import temporal_host_loop
from tests.denoise_cases import F, same_bits
from tests.helpers import ROOT, host_api_source
from tests.temporal_cases import frame_params
from tests.temporal_split_cases import split_frame, split_frame_odd, static_split_frames

NEW = ("rr_accumulate_split_records_device", "rr_accumulate_split_records")
KINDS = {"clean": split_frame, "odd": split_frame_odd}
KEYS = ("records", "length", "halves", "diffuse", "diffuse_halves")


@pytest.fixture(scope="module")
def host_loop(tmp_path_factory):
    exe = temporal_host_loop.build(tmp_path_factory)

    def run(tmp_path, cam, prm, records, halves, diffuse, diffuse_halves, history, history_halves, history_diffuse, history_diffuse_halves, history_length, motion):
        return temporal_host_loop.run(exe, tmp_path, cam, prm, None, True, (records, halves, diffuse, diffuse_halves, history, history_halves, history_diffuse,
                                                                            history_diffuse_halves, history_length, motion))
    return run


def _same(got, want, what, keys=KEYS):
    for key in keys:
        if want[key] is None:
            assert got[key] is None
            continue
        g, w = np.ascontiguousarray(got[key]).view(np.uint32), np.ascontiguousarray(want[key]).view(np.uint32)
        assert same_bits(g, w), f"{what}: {int((g != w).sum())} words of {key} differ"


def _inputs(case, use_halves, use_motion, first):
    """the twelve array arguments of accumulate_split_records, in its order"""
    hv = case["halves"] if use_halves else None
    dh = case["diffuse_halves"] if use_halves else None
    mv = case["motion"] if use_motion else None
    if first:
        return case["records"], hv, case["diffuse"], dh, None, None, None, None, None, mv
    return (case["records"], hv, case["diffuse"], dh, case["history"], case["history_halves"] if use_halves else None, case["history_diffuse"],
            case["history_diffuse_halves"] if use_halves else None, case["history_length"], mv)


def _plain(args):
    """of _inputs: the arguments of accumulate_records"""
    rec, hv, _, _, hist, hist_h, _, _, hist_l, mv = args
    return rec, hv, hist, hist_h, hist_l, mv


def held_share(got, current):
    """of the kept pixels (length > 1): the share whose diffuse layer nevertheless holds its current bits, per layer"""
    kept = got["length"] > 1
    layers = [(got["diffuse"], current["diffuse"])]
    if got["diffuse_halves"] is not None:
        layers += [(got["diffuse_halves"][:, h], current["diffuse_halves"][:, h]) for h in (0, 1)]
    return [float((same(g, c) & kept).sum() / max(int(kept.sum()), 1)) for g, c in layers for same in [lambda a, b: (
        np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all(-1)]]


@pytest.mark.parametrize("size", [(33, 9), (37, 19), (130, 70)])
def test_the_odd_case_has_what_it_promises(size):
    """A condition on the inputs: in the yardstick's answer some, and fewer than one in ten, of the kept pixels hold their current diffuse
    bits, in every layer -- the rule 'a non-finite triple or history mean restarts the layer' is exercised and hides nothing.  On the
    clean case only a blend that happens to return its input could do that."""
    odd, clean = split_frame_odd(*size), split_frame(*size)
    assert not same_bits(odd["diffuse"], clean["diffuse"]) and not same_bits(odd["history_diffuse"], clean["history_diffuse"])
    for name in ("records", "halves", "history", "history_halves", "history_length", "motion"):
        assert same_bits(odd[name], clean[name])
    # broken only where the colour is finite
    for d, c in ((odd["diffuse"], odd["records"][:, 0:3]), (odd["history_diffuse"], odd["history"][:, 0:3])):
        assert (~np.isfinite(d).all(-1) & np.isfinite(c).all(-1)).any() and np.isnan(d).any() and np.isinf(d).any()
    for use_halves in (True, False):
        for use_motion in (True, False):
            shares = held_share(accumulate_split_records(*_inputs(odd, use_halves, use_motion, False), odd["cam"], frame_params(odd)), odd)
            print(size, use_halves, use_motion, shares)
            assert all(0 < s < 0.1 for s in shares), shares
            none = held_share(accumulate_split_records(*_inputs(clean, use_halves, use_motion, False), clean["cam"], frame_params(clean)), clean)
            assert all(s < 0.01 for s in none), none


CONFIGS = [(True, True, 1 / 64, False), (True, False, 0.0, False), (False, True, 0.0, False), (False, False, 1 / 64, False),
           (True, True, 1 / 64, True), (False, False, 0.0, True), (True, False, 1 / 64, False), (False, True, 1 / 64, True)]


@pytest.mark.parametrize("kind", ["clean", "odd"])
@pytest.mark.parametrize("size", [(37, 19), (130, 70)])
@pytest.mark.parametrize("use_halves,use_motion,snap,first", CONFIGS)
def test_host_loop_equals_the_yardstick(host_loop, tmp_path, kind, size, use_halves, use_motion, snap, first):
    case = KINDS[kind](*size)
    prm = frame_params(case, snap=snap)
    args = _inputs(case, use_halves, use_motion, first)
    want = accumulate_split_records(*args, case["cam"], prm)
    _same(host_loop(tmp_path, case["cam"], prm, *args), want, f"{kind} {size} halves={use_halves} motion={use_motion} snap={snap} first={first}")
    if first:
        assert same_bits(want["diffuse"], case["diffuse"]) and (not use_halves or same_bits(want["diffuse_halves"], case["diffuse_halves"]))


@pytest.mark.parametrize("kind", ["clean", "odd"])
@pytest.mark.parametrize("size", [(37, 19), (130, 70)])
@pytest.mark.parametrize("use_halves,use_motion,snap,first", CONFIGS[:6])
def test_records_halves_and_length_are_those_of_accumulate_records(kind, size, use_halves, use_motion, snap, first):
    """Identity 1: whatever the diffuse holds."""
    case = KINDS[kind](*size)
    prm = frame_params(case, snap=snap)
    args = _inputs(case, use_halves, use_motion, first)
    got, want = accumulate_split_records(*args, case["cam"], prm), accumulate_records(*_plain(args), case["cam"], prm)
    _same(got, want, f"{kind} {size}", keys=("records", "length", "halves"))
    for key in ("x", "y", "weight", "taken", "reprojected"):
        assert same_bits(got["taps"][key], want["taps"][key])


@pytest.mark.parametrize("size", [(37, 19), (130, 70)])
@pytest.mark.parametrize("use_halves,use_motion,snap", [(True, True, 1 / 64), (True, False, 0.0), (False, True, 0.0), (False, False, 1 / 64)])
def test_a_diffuse_layer_is_what_accumulate_records_makes_of_it_as_a_colour(size, use_halves, use_motion, snap):
    """Identity 2, on the clean case (a diffuse triple is finite exactly when its colour is, so the decisions agree): records whose colour
    is replaced by the diffuse, under a history whose colour is replaced by the history diffuse -- depth, normal, id and length the same --
    accumulate to the diffuse output.  The new yardstick is held to the old one."""
    case = split_frame(*size)
    prm = frame_params(case, snap=snap)
    args = _inputs(case, use_halves, use_motion, False)
    got = accumulate_split_records(*args, case["cam"], prm)

    def swapped(records, diffuse):
        if records is None:
            return None
        out = np.array(records, F)
        out[..., 0:3] = diffuse
        return out
    rec, hv, df, dh, hist, hist_h, hist_d, hist_dh, hist_l, mv = args
    want = accumulate_records(swapped(rec, df), swapped(hv, dh), swapped(hist, hist_d), swapped(hist_h, hist_dh), hist_l, mv, case["cam"], prm)
    assert same_bits(want["length"], got["length"])
    assert same_bits(got["diffuse"], np.ascontiguousarray(want["records"][:, 0:3]))
    if use_halves:
        assert same_bits(got["diffuse_halves"], np.ascontiguousarray(want["halves"][:, :, 0:3]))
    assert (got["length"] > 1).sum() > 100 and not same_bits(got["diffuse"], case["diffuse"])


# ---- a static view ---------------------------------------------------------------------------------------------------------------
def _feed(cam, prm, records, halves, diffuse, diffuse_halves):
    st = dict(records=None, halves=None, diffuse=None, diffuse_halves=None, length=None)
    for k in range(len(records)):
        st = accumulate_split_records(records[k], halves[k], diffuse[k], diffuse_halves[k], st["records"], st["halves"], st["diffuse"], st["diffuse_halves"],
                                      st["length"], None, cam, prm)
        yield st


def test_host_loop_equals_the_yardstick_on_the_static_view(host_loop, tmp_path):
    cam, prm, records, halves, diffuse, diffuse_halves = static_split_frames(37, 19, 2)
    first = accumulate_split_records(records[0], halves[0], diffuse[0], diffuse_halves[0], None, None, None, None, None, None, cam, prm)
    args = (records[1], halves[1], diffuse[1], diffuse_halves[1], first["records"], first["halves"], first["diffuse"], first["diffuse_halves"], first["length"], None)
    _same(host_loop(tmp_path, cam, prm, *args), accumulate_split_records(*args, cam, prm), "static view")


def test_a_static_camera_forms_the_mean_of_six_frames():
    """Every pixel reaches length 6; the accumulated diffuse lies within 6 * 2^-22 * max|d| of the float64 mean (the bound
    tests/test_gpu_temporal.py derives for colour: per step a division, a difference, a product and a sum, each rounded by at most 2^-24
    of the largest value), and accumulated colour - accumulated diffuse within twice that bound (of the colours) of the float64 mean of
    colour - diffuse: both terms carry their own error."""
    cam, prm, records, halves, diffuse, diffuse_halves = static_split_frames(37, 19, 6)
    st = list(_feed(cam, prm, records, halves, diffuse, diffuse_halves))[-1]
    assert (st["length"] == 6).all()
    layers = ((st["records"][:, 0:3], st["diffuse"], records[:, :, 0:3], diffuse), (st["halves"][:, 0, 0:3], st["diffuse_halves"][:, 0], halves[:, :, 0, 0:3], diffuse_halves[:, :, 0]),
              (st["halves"][:, 1, 0:3], st["diffuse_halves"][:, 1], halves[:, :, 1, 0:3], diffuse_halves[:, :, 1]))
    for got_c, got_d, frames_c, frames_d in layers:
        bound_d = 6 * 2.0 ** -22 * float(np.abs(frames_d).max())
        err_d = float(np.abs(got_d.astype(np.float64) - frames_d.astype(np.float64).mean(0)).max())
        bound_r = 2 * 6 * 2.0 ** -22 * float(np.abs(frames_c).max())
        rest = got_c.astype(np.float64) - got_d.astype(np.float64)
        err_r = float(np.abs(rest - (frames_c.astype(np.float64) - frames_d.astype(np.float64)).mean(0)).max())
        print(f"diffuse: deviation {err_d:.3g}, bound {bound_d:.3g}; rest: deviation {err_r:.3g}, bound {bound_r:.3g}")
        assert err_d <= bound_d and err_r <= bound_r
        assert float(np.abs(got_d).max()) > 0 and not np.array_equal(got_d, got_c)


def test_a_static_camera_keeps_a_repeated_frame_bit_for_bit():
    cam, prm, records, halves, diffuse, diffuse_halves = static_split_frames(37, 19, 1)
    feed = _feed(cam, prm, [records[0]] * 40, [halves[0]] * 40, [diffuse[0]] * 40, [diffuse_halves[0]] * 40)
    for k, st in enumerate(feed, start=1):
        assert same_bits(st["records"], records[0]) and same_bits(st["halves"], halves[0]), k
        assert same_bits(st["diffuse"], diffuse[0]) and same_bits(st["diffuse_halves"], diffuse_halves[0]), k
        assert (st["length"] == min(k, 32)).all(), k


def test_the_yardstick_refuses_unpaired_arguments():
    case = split_frame(37, 19)
    a = list(_inputs(case, True, False, False))
    for drop in (2, 3, 6, 7):
        bad = list(a)
        bad[drop] = None
        with pytest.raises(ValueError):
            accumulate_split_records(*bad, case["cam"], frame_params(case))


# ---- the entry points, without a device -----------------------------------------------------------------------------------------
def test_refusals_without_a_device():
    """Every call below is refused on its arguments alone, before the scene is looked at: the made-up handle is never dereferenced."""
    L = capi.lib()
    W, H = 20, 12
    n = W * H
    rec, hist = np.full((n + 4, 8), 0.5, F), np.full((n + 4, 8), 0.5, F)
    halves, hist_h = np.full((n + 4, 2, 8), 0.5, F), np.full((n + 4, 2, 8), 0.5, F)
    # (every diffuse array is as long as the longest output, 64 n bytes and more: an output laid over one overlaps that one alone)
    dif, hist_d = np.full((6 * n, 3), 0.25, F), np.full((6 * n, 3), 0.25, F)
    dif_h, hist_dh = np.full((3 * n, 2, 3), 0.25, F), np.full((3 * n, 2, 3), 0.25, F)
    hist_l, motion = np.full(n + 4, 1.0, F), np.zeros((n + 4, 3), F)
    out, out_h = np.full((n + 4, 8), 7.0, F), np.full((n + 4, 2, 8), 7.0, F)
    out_d, out_dh = np.full((6 * n, 3), 7.0, F), np.full((3 * n, 2, 3), 7.0, F)
    length, rgba = np.full(n + 4, 7.0, F), np.full((n + 4, 4), 0x5a, np.uint8)
    fake = C.c_void_p(0x1000)
    P = lambda a, off=0: C.c_void_p(a.ctypes.data + off)
    good = capi.accumulate_default_params

    for name, dev in (("rr_accumulate_split_records", False), ("rr_accumulate_split_records_device", True)):
        fn = getattr(L, name)

        def call(scene=fake, w=W, h=H, prm=None, r=P(rec), hv=P(halves), d=P(dif), dh=P(dif_h), hi=P(hist), hh=P(hist_h), hd=P(hist_d), hdh=P(hist_dh),
                 hl=P(hist_l), mv=P(motion), o=P(out), oh=P(out_h), od=P(out_d), odh=P(out_dh), lo=P(length), rg=P(rgba), null_prm=False, null_cam=False):
            p = prm or good()
            c = capi.rr_camera()
            c.width, c.height = w, h
            args = [scene, None if null_cam else C.byref(c), None if null_prm else C.byref(p), r, hv, d, dh, hi, hh, hd, hdh, hl, mv, o, oh, od, odh, lo, rg]
            return fn(*(args + [None] if dev else args))

        err = lambda: L.rr_last_error()
        assert call(scene=None) == -1 and b"scene" in err()
        assert call(null_cam=True) == -1 and b"camera" in err()
        assert call(null_prm=True) == -1 and b"params" in err()
        assert call(r=None) == -1 and b"records" in err()
        assert call(o=None) == -1 and b"out is NULL" in err()
        assert call(lo=None) == -1 and b"length_out" in err()
        assert call(d=None) == -1 and b"diffuse is NULL" in err()
        assert call(od=None) == -1 and b"diffuse_out is NULL" in err()
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
        # what comes with what: the rules of rr_accumulate_records ...
        assert call(hi=None, hd=None) == -1 and b"history and history_length" in err()
        assert call(hl=None) == -1 and b"history and history_length" in err()
        assert call(hh=None, hdh=None) == -1 and b"history_halves" in err()
        assert call(oh=None) == -1 and b"halves_out is required" in err()
        # ... and the diffuse layers'
        assert call(dh=None) == -1 and b"diffuse_halves is required exactly when halves" in err()
        assert call(hv=None, oh=None, hh=None, hdh=None, odh=None) == -1 and b"diffuse_halves is required exactly when halves" in err()
        assert call(odh=None) == -1 and b"diffuse_halves_out is required exactly when halves" in err()
        assert call(hv=None, oh=None, hh=None, hdh=None, dh=None) == -1 and b"diffuse_halves_out is required exactly when halves" in err()
        assert call(hd=None) == -1 and b"history_diffuse is required exactly when history" in err()
        assert call(hi=None, hl=None, hh=None, hdh=None) == -1 and b"history_diffuse is required exactly when history" in err()
        assert call(hdh=None) == -1 and b"history_diffuse_halves is required exactly when history_halves" in err()
        assert call(hi=None, hl=None, hh=None, hd=None) == -1 and b"history_diffuse_halves is required exactly when history_halves" in err()
        # overlaps: only the four in-place pairs are allowed
        assert call(o=P(rec, 32)) == -1 and b"out overlaps records" in err()
        assert call(o=P(hist)) == -1 and b"out overlaps history" in err()
        assert call(oh=P(halves, 32)) == -1 and b"halves_out overlaps halves" in err()
        assert call(od=P(dif, 12)) == -1 and b"diffuse_out overlaps diffuse" in err() and b"in place" in err()
        assert call(od=P(hist_d)) == -1 and b"diffuse_out overlaps history_diffuse" in err()
        assert call(od=P(dif_h)) == -1 and b"diffuse_out overlaps diffuse_halves" in err()
        assert call(od=P(rec)) == -1 and b"diffuse_out overlaps records" in err()
        assert call(odh=P(dif_h, 12)) == -1 and b"diffuse_halves_out overlaps diffuse_halves" in err()
        assert call(odh=P(hist_dh)) == -1 and b"diffuse_halves_out overlaps history_diffuse_halves" in err()
        assert call(odh=P(dif)) == -1 and b"diffuse_halves_out overlaps diffuse " in err()
        assert call(odh=P(hist_h)) == -1 and b"diffuse_halves_out overlaps history_halves" in err()
        assert call(o=P(dif)) == -1 and b"out overlaps diffuse" in err()
        assert call(oh=P(hist_dh)) == -1 and b"halves_out overlaps history_diffuse_halves" in err()
        assert call(lo=P(hist_d)) == -1 and b"length_out overlaps history_diffuse" in err()
        assert call(rg=P(dif_h)) == -1 and b"rgba8_out overlaps diffuse_halves" in err()
        assert call(od=P(out)) == -1 and b"out overlaps diffuse_out" in err()
        assert call(odh=P(out_d)) == -1 and b"diffuse_out overlaps diffuse_halves_out" in err()
        assert call(lo=P(out_dh)) == -1 and b"diffuse_halves_out overlaps length_out" in err()
        assert call(rg=P(out_d)) == -1 and b"diffuse_out overlaps rgba8_out" in err()
        if dev:   # the alignment rules of the device form
            for kw in (dict(r=P(rec, 8)), dict(hv=P(halves, 4)), dict(hi=P(hist, 8)), dict(hh=P(hist_h, 8)), dict(o=P(out, 8)), dict(oh=P(out_h, 4))):
                assert call(**kw) == -1 and b"16-byte aligned" in err(), kw
            for kw in (dict(hl=P(hist_l, 2)), dict(mv=P(motion, 1)), dict(lo=P(length, 2)), dict(rg=P(rgba, 1)), dict(d=P(dif, 2)), dict(dh=P(dif_h, 1)),
                       dict(hd=P(hist_d, 3)), dict(hdh=P(hist_dh, 2)), dict(od=P(out_d, 2)), dict(odh=P(out_dh, 1))):
                assert call(**kw) == -1 and b"4-byte aligned" in err(), kw
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
    assert len(capi.lib().rr_accumulate_split_records.argtypes) == 19 and len(capi.lib().rr_accumulate_split_records_device.argtypes) == 20
    header = open(os.path.join(ROOT, "include", "rustray_hip.h")).read()
    for n in NEW:
        assert re.search(r'^int ' + n + r'\(', header, re.M)
    # the staging pool has a slot per argument of the call with the most
    handle = open(os.path.join(ROOT, "rustray_amd", "csrc", "rr_api_handle.h")).read()
    assert re.search(r"struct RecordStage \{\s*DevBuf buf\[16\];", handle)
    # rr_temporal.h stays plain host logic
    text = open(os.path.join(ROOT, "rustray_amd", "csrc", "rr_temporal.h")).read()
    assert re.findall(r'#include\s+(\S+)', text) == ['"rr_denoise.h"', '"rr_pixel_list.h"']
    for m in ("accumulate_split", "accumulate_split_device"):
        assert hasattr(capi.DeviceScene, m)
    from rustray_amd import renderer
    assert hasattr(renderer, "accumulate_split_torch") and hasattr(renderer, "render_temporal_split_torch")
    assert hasattr(renderer.Raytracing, "render_temporal_split")
