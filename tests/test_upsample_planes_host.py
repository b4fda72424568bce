"""rr_upsample_albedo_records without a GPU: the yardstick with albedo planes against itself on guides whose base colour was overwritten
by the planes, bit for bit; the host loop over rustray_amd/csrc/rr_upsample.h with the guides loaded the way the kernel's planes build
loads them, under AddressSanitizer + UBSan, against the yardstick; the quality of mean albedo planes on a box-averaged frame; what the
entry points refuse before they touch a device; the bindings' argument order against the header's parameter names; the pipelines'
argument checks.

(The module's name sorts behind tests/test_upsample_host.py on purpose.  That module's refusal test hands the library a halves_out range
four times the size of the numpy array it starts in and expects the conflict with halves_low to be named; which array lies behind
`halves` is the allocator's choice, and when it is `out` the library names that pair first, as its search order says.  Tests that run
just before it and free arrays of its sizes shift that choice, so these run behind it; the refusal test here carves its buffers from one
allocation for the same reason.)"""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from rustray_amd import capi
from rustray_amd.flat import SURFACE_HIT_DTYPE
from rustray_amd.upsample import UpsampleParams, upsample_records
from tests.denoise_cases import F, differing_words
from tests.helpers import ROOT, host_api_source
from tests.test_temporal_binding_host import HANDLE, _address, _header, _one_call, _param_names, recorder, scene  # noqa: F401 (fixtures)
from tests.upsample_albedo_cases import PLANE_SETS, box_quality_case, guide_with, random_planes
from tests.upsample_cases import SHAPES, random_case

NEW = ("rr_upsample_albedo_records_device", "rr_upsample_albedo_records")
ids = lambda s: "%dx%d_from_%dx%d" % s


def _same(got, want, what):
    """every word of records and weight; the halves by the NaN-aware comparison (a NaN the arithmetic generates has no specified bits)"""
    for key in ("records", "weight"):
        g, w = got[key].view(np.uint32), want[key].view(np.uint32)
        assert g.shape == w.shape and np.array_equal(g, w), f"{what}: {int((g != w).sum())} words of {key} differ"
    if want["halves"] is None:
        assert got["halves"] is None, what
    else:
        differ, nans = differing_words(got["halves"], want["halves"])
        assert differ == 0, f"{what}: {differ} half words differ ({nans} are NaNs of other bits on both sides)"


def _variants(power):
    for use_halves in (True, False):
        yield use_halves, UpsampleParams(normal_power_log2=power, sigma_depth=0.05 if power else 0.3)


def test_the_planes_hold_what_they_promise():
    W, H, w, h = SHAPES[0]
    _, _, guide_low, guide = random_case(W, H, w, h)
    for plane, g in zip(random_planes(W, H, w, h), (guide_low, guide)):
        hit = g["hit"] != 0
        assert (~hit).any() and np.isnan(plane[~hit]).all()
        a = plane[hit]
        assert (a == 0).any() and (a == F(2.0 ** -10)).any() and (a == np.nextafter(F(2.0 ** -10), F(1))).any()
        assert np.isnan(a).any() and np.isposinf(a).any() and (a < 0).any()
        ordinary = a[np.isfinite(a) & (a > F(2.0 ** -9))]
        assert ordinary.min() >= F(0.05) and ordinary.max() < F(1.05)
        assert not np.array_equal(plane[hit], g["base_color"][hit][:, 0:3])
    small = random_planes(*SHAPES[3])
    assert small[0].shape == (1, 3) and small[1].shape == (1, 3)


# ---- the yardstick --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
@pytest.mark.parametrize("power", (0, 5, 7))
def test_planes_equal_guides_overwritten_by_them(shape, power):
    W, H, w, h = shape
    low, halves, guide_low, guide = random_case(W, H, w, h)
    planes = random_planes(W, H, w, h)
    for use_halves, prm in _variants(power):
        hv = halves if use_halves else None
        plain = upsample_records(low, hv, guide_low, guide, w, h, W, H, prm)
        _same(upsample_records(low, hv, guide_low, guide, w, h, W, H, prm, albedo_low=None, albedo=None), plain, f"{shape}: both planes None")
        off = UpsampleParams(normal_power_log2=power, sigma_depth=prm.sigma_depth, use_albedo=False)
        plain_off = upsample_records(low, hv, guide_low, guide, w, h, W, H, off)
        for name, with_low, with_full in PLANE_SETS:
            al, af = (planes[0] if with_low else None), (planes[1] if with_full else None)
            what = f"{shape} power {power} halves={use_halves} planes={name}"
            got = upsample_records(low, hv, guide_low, guide, w, h, W, H, prm, albedo_low=al, albedo=af)
            _same(got, upsample_records(low, hv, guide_with(guide_low, al), guide_with(guide, af), w, h, W, H, prm), what)
            # the value of a plane at a pixel that is not a hit reaches no result
            zl, zf = (None if al is None else np.where(np.isnan(al) & (guide_low["hit"] == 0)[:, None], F(0), al),
                      None if af is None else np.where(np.isnan(af) & (guide["hit"] == 0)[:, None], F(0), af))
            _same(upsample_records(low, hv, guide_low, guide, w, h, W, H, prm, albedo_low=zl, albedo=zf), got, what + ", zeros at the misses")
            _same(upsample_records(low, hv, guide_low, guide, w, h, W, H, off, albedo_low=al, albedo=af), plain_off, what + ", use_albedo off")
        if w * h >= 64:   # (the planes are not the guides' own colours: the identity above is not a vacuous one)
            both = upsample_records(low, hv, guide_low, guide, w, h, W, H, prm, albedo_low=planes[0], albedo=planes[1])
            assert not np.array_equal(both["records"].view(np.uint32), plain["records"].view(np.uint32))


def test_a_plane_of_the_wrong_size_is_refused():
    W, H, w, h = SHAPES[0]
    low, halves, guide_low, guide = random_case(W, H, w, h)
    al, af = random_planes(W, H, w, h)
    with pytest.raises(ValueError, match="albedo_low"):
        upsample_records(low, halves, guide_low, guide, w, h, W, H, albedo_low=af)
    with pytest.raises(ValueError, match="albedo"):
        upsample_records(low, halves, guide_low, guide, w, h, W, H, albedo=al)


# ---- the host loop --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_loop(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("upsample_albedo") / "upsample_albedo_test")
    cmd = ["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-o", exe, os.path.join(ROOT, "tests", "native", "upsample_albedo_test.cpp")]
    subprocess.check_call(cmd)

    def run(tmp_path, w, h, W, H, low, halves, guide_low, guide, albedo_low, albedo, prm):
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(src, "wb") as fh:
            fh.write(struct.pack("<7If2I", w, h, W, H, halves is not None, prm.normal_power_log2, bool(prm.use_albedo), prm.sigma_depth, albedo_low is not None,
                                 albedo is not None))
            for a in (low, halves):
                if a is not None:
                    fh.write(np.ascontiguousarray(a, F).tobytes())
            fh.write(guide_low.tobytes())
            fh.write(guide.tobytes())
            for a in (albedo_low, albedo):
                if a is not None:
                    fh.write(np.ascontiguousarray(a, F).tobytes())
        out = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and "upsample albedo test OK" in out.stdout, out.stdout + out.stderr
        raw = np.fromfile(dst, F)
        n, k = W * H, (24 if halves is not None else 8)
        assert raw.size == (k + 1) * n
        return dict(records=raw[:8 * n].reshape(n, 8), halves=raw[8 * n:k * n].reshape(n, 2, 8) if halves is not None else None, weight=raw[k * n:])
    return run


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_host_loop_equals_the_yardstick(host_loop, tmp_path, shape):
    W, H, w, h = shape
    low, halves, guide_low, guide = random_case(W, H, w, h)
    planes = random_planes(W, H, w, h)
    for power in (0, 5, 7):
        for use_halves, prm in _variants(power):
            hv = halves if use_halves else None
            for name, with_low, with_full in PLANE_SETS + (("none", False, False),):
                al, af = (planes[0] if with_low else None), (planes[1] if with_full else None)
                _same(host_loop(tmp_path, w, h, W, H, low, hv, guide_low, guide, al, af, prm),
                      upsample_records(low, hv, guide_low, guide, w, h, W, H, prm, albedo_low=al, albedo=af), f"{shape} power {power} halves={use_halves} planes={name}")
    off = UpsampleParams(use_albedo=False)
    _same(host_loop(tmp_path, w, h, W, H, low, halves, guide_low, guide, planes[0], planes[1], off),
          upsample_records(low, halves, guide_low, guide, w, h, W, H, off, albedo_low=planes[0], albedo=planes[1]), f"{shape} use_albedo off")


# ---- quality ----------------------------------------------------------------------------------------------------------------------------
def test_mean_planes_on_a_box_averaged_frame():
    """64x48 <- 32x24, quality_case's scene with every pixel's colour and albedo averaged over its footprint, as sub-samples make them
    (tests/upsample_albedo_cases.py: box_quality_case), default parameters.  Demodulating the low frame by its mean albedo repairs the
    quotient, and remodulating by the full frame's mean albedo is a further step: MSE against the averaged full-resolution truth
    centre / centre 3.954e-04, mean / centre 1.382e-04, mean / mean 1.623e-05 (this yardstick; recorded in DESIGN.md)."""
    truth, low, guide_low, guide, mean_low, mean_full = box_quality_case()
    run = lambda **kw: upsample_records(low, None, guide_low, guide, 32, 24, 64, 48, **kw)
    mse = lambda res: float(np.mean((res["records"][:, 0:3].astype(np.float64) - truth) ** 2))
    centre, mean_centre, mean_mean = run(), run(albedo_low=mean_low), run(albedo_low=mean_low, albedo=mean_full)
    figures = f"MSE centre / centre {mse(centre):.3e}, mean / centre {mse(mean_centre):.3e}, mean / mean {mse(mean_mean):.3e}"
    print(figures)
    for res in (centre, mean_centre, mean_mean):
        assert (res["weight"] > 0).all(), "a pixel has weight 0"
    assert mse(mean_mean) <= 0.25 * mse(centre), figures
    assert mse(mean_centre) < mse(centre), figures


# ---- the entry points, without a device -------------------------------------------------------------------------------------------------
def test_refusals_without_a_device():
    """Every call below is refused on its arguments alone, before the scene is looked at: the made-up handle is never dereferenced.  A
    call that passes every check here reaches the scene, so the calls that must be ACCEPTED by a check are shown by the refusal that comes
    after it in the header's order: the size of the frame (2^30), which is the last."""
    L = capi.lib()
    w, h, W, H = 10, 6, 20, 12
    nl, n = w * h, W * H
    # every buffer is a view into ONE allocation, 32 KiB apart at least: which ranges overlap is then decided here and not by the allocator
    arena = np.zeros(1 << 20, np.uint8)
    at = [(-arena.ctypes.data) % 64]

    def carve(shape, dtype, fill):
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        a = arena[at[0]:at[0] + nbytes].view(dtype).reshape(shape)
        at[0] += (nbytes + (32 << 10) + 63) // 64 * 64
        a[...] = fill
        return a

    low, halves = carve((nl, 8), F, 0.5), carve((nl, 2, 8), F, 0.5)
    guide_low, guide = carve((nl + 1,), SURFACE_HIT_DTYPE, 0), carve((n + 1,), SURFACE_HIT_DTYPE, 0)
    al, af = carve((nl + 2, 3), F, 0.5), carve((n + 2, 3), F, 0.5)
    out, hout = carve((n + 4, 8), F, 7.0), carve((n + 4, 2, 8), F, 7.0)
    rgba, wt = carve((n + 4, 4), np.uint8, 0x5a), carve((n + 4,), F, 7.0)
    assert at[0] <= arena.size
    fake = C.c_void_p(0x1000)
    P = lambda a, off=0: C.c_void_p(a.ctypes.data + off)
    good = capi.upsample_default_params
    err = lambda: L.rr_last_error()

    for name, dev in (("rr_upsample_albedo_records", False), ("rr_upsample_albedo_records_device", True)):
        fn = getattr(L, name)

        def call(scene=fake, lw=w, lh=h, fw=W, fh=H, prm=None, lo=P(low), hv=P(halves), gl=P(guide_low), gf=P(guide), pl=P(al), pf=P(af), o=P(out), ho=P(hout),
                 rg=P(rgba), wo=P(wt), null_prm=False):
            p = prm or good()
            args = [scene, lw, lh, fw, fh, None if null_prm else C.byref(p), lo, hv, gl, gf, pl, pf, o, ho, rg, wo]
            return fn(*(args + [None] if dev else args))

        for planes in (dict(pl=None, pf=None), dict()):      # the existing order, with the planes NULL and with them given
            k = lambda **kw: call(**dict(planes, **kw))
            assert k(scene=None) == -1 and b"scene" in err()
            assert k(null_prm=True) == -1 and b"params" in err()
            for kw, word in ((dict(lo=None), b"low is NULL"), (dict(gl=None), b"guide_low is NULL"), (dict(gf=None), b"guide is NULL"), (dict(o=None), b"out is NULL")):
                assert k(**kw) == -1 and word in err(), (name, kw, err())
            assert k(fw=0) == -1 and k(fh=65536) == -1 and b"frame size" in err()
            assert k(lw=0) == -1 and k(lh=H + 1) == -1 and b"low frame size" in err()
            for field, val in (("struct_size", 16), ("normal_power_log2", 8), ("sigma_depth", float("nan"))):
                p = good()
                setattr(p, field, val)
                assert k(prm=p) == -1 and field.encode() in err(), (name, field, err())
            assert k(hv=None) == -1 and b"together" in err()
            assert k(ho=None) == -1 and b"together" in err()
            # each refusal comes before the ones after it: a NULL low with a bad size, a bad size with a bad struct, ... , an overlap
            assert k(lo=None, fw=0) == -1 and b"low is NULL" in err()
            p = good()
            p.struct_size = 0
            assert k(fw=0, prm=p) == -1 and b"frame size" in err()
            assert k(prm=p, hv=None) == -1 and b"struct_size" in err()
            if dev:
                assert k(hv=None, lo=P(low, 8)) == -1 and b"together" in err()
                assert k(lo=P(low, 8), wo=P(wt, 2)) == -1 and b"16-byte aligned" in err()
                assert k(rg=P(rgba, 1)) == -1 and k(wo=P(wt, 2)) == -1 and b"4-byte aligned" in err()
                assert k(wo=P(wt, 2), o=P(low)) == -1 and b"4-byte aligned" in err()
            assert k(o=P(low)) == -1 and b"out overlaps low" in err()
            assert k(ho=P(halves)) == -1 and b"halves_out overlaps halves_low" in err()
            assert k(rg=P(guide_low)) == -1 and b"rgba8_out overlaps guide_low" in err()
            assert k(wo=P(out, 32 * n - 16)) == -1 and b"out overlaps weight_out" in err()
            assert k(ho=P(out, 64)) == -1 and b"out overlaps halves_out" in err()

        # more than 2^30 half records: the last refusal, so the made-up buffers lie 2^40 bytes apart and overlap nothing
        far = lambda k, off=0: C.c_void_p(((k + 1) << 40) + off)
        big = dict(lw=1, lh=1, fw=32768, fh=16385, lo=far(0), hv=far(1), gl=far(2), gf=far(3), o=far(4), ho=far(5), rg=far(6), wo=far(7), pl=far(8), pf=far(9))
        assert call(**big) == -2 and b"2^30" in err()
        # a plane at an address = 2 (mod 4): refused in the device form, accepted in the host form
        for kw in (dict(pl=far(8, 2)), dict(pf=far(9, 2))):
            if dev:
                assert call(**dict(big, **kw)) == -1 and b"4-byte aligned" in err() and b"albedo" in err(), (name, kw, err())
            else:
                assert call(**dict(big, **kw)) == -2 and b"2^30" in err(), (name, kw, err())
        # a plane that is 4-byte and not 16-byte aligned is accepted by both
        assert call(**dict(big, pl=far(8, 4), pf=far(9, 12))) == -2 and b"2^30" in err()
        # a plane over an output is refused by name
        for plane, key, bytes_of in (("albedo_low", "pl", 12), ("albedo", "pf", 12 * 32768 * 16385)):
            for o_name, o_key, slot in (("out", "o", 4), ("halves_out", "ho", 5), ("rgba8_out", "rg", 6), ("weight_out", "wo", 7)):
                assert call(**dict(big, **{key: far(slot)})) == -1 and f"{o_name} overlaps {plane}".encode() in err(), (name, plane, o_name, err())
            assert call(**dict(big, **{key: far(4, -bytes_of + 4)})) == -1 and f"out overlaps {plane}".encode() in err()      # by its last float
            assert call(**dict(big, **{key: far(4, -bytes_of)})) == -2 and b"2^30" in err()                                     # touching is no overlap
        # the planes are inputs: over guide_low, over each other and over any other input they pass this check
        assert call(**dict(big, pl=far(2))) == -2 and b"2^30" in err()
        assert call(**dict(big, pl=far(9))) == -2 and b"2^30" in err()
        assert call(**dict(big, pl=far(0), pf=far(3, 16))) == -2 and b"2^30" in err()
        assert call(**dict(big, wo=far(4))) == -1 and b"overlaps" in err()
    assert (out == 7.0).all() and (hout == 7.0).all() and (rgba == 0x5a).all() and (wt == 7.0).all()


def test_the_new_entry_points_are_guarded_declared_and_bound():
    src = host_api_source()
    hdr = _header()
    for name in NEW:
        assert re.search(r'^int ' + name + r'\([^{]*\) try \{', src, re.M), f"{name} is not a function-try-block"
        assert f'RR_GUARD_END("{name}")' in src
        assert re.search(r"\bint " + name + r"\s*\(", hdr), f"{name} is not declared"
        assert name in capi.EXPORTS and hasattr(capi.lib(), name) and getattr(capi.lib(), name).argtypes is not None
    # one check, one body: the older pair is the new one with two NULLs
    api = open(os.path.join(ROOT, "rustray_amd", "csrc", "rr_api_upsample.h")).read()
    assert len(re.findall(r"^static int check_upsample_args\(", api, re.M)) == 1 and len(re.findall(r"^static int upsample_locked\(", api, re.M)) == 1
    assert len(re.findall(r"check_arg_ranges\(", api)) == 1 and "const ArgRange t[10]" in api
    whole = open(os.path.join(ROOT, "include", "rustray_hip.h")).read()
    assert "rr_upsample_albedo_records and rr_upsample_albedo_records_device came after those" in whole and "#define RR_ABI_VERSION 3u" in whole
    shim = open(os.path.join(ROOT, "rustray_amd", "csrc", "host_shim.cpp")).read()
    assert 'extern "C" int rh_upsample_albedo(' in shim


# ---- the bindings' argument order against the header's parameter names ----------------------------------------------------------------------
def test_device_form_passes_every_argument_in_the_headers_order(recorder, scene):
    names = _param_names(_header(), "rr_upsample_albedo_records_device")
    assert names == ["scene", "low_width", "low_height", "width", "height", "params", "low_dev", "halves_low_dev", "guide_low_dev", "guide_dev", "albedo_low_dev",
                     "albedo_dev", "out_dev", "halves_out_dev", "rgba8_out_dev", "weight_out_dev", "hip_stream"]
    keyword = dict(low_dev="low_ptr", halves_low_dev="halves_low_ptr", guide_low_dev="guide_low_ptr", guide_dev="guide_ptr", albedo_low_dev="albedo_low",
                   albedo_dev="albedo", out_dev="out_ptr", halves_out_dev="halves_out_ptr", rgba8_out_dev="rgba8_ptr", weight_out_dev="weight_out_ptr",
                   hip_stream="stream_ptr")
    prm = capi.rr_upsample_params()
    values = {kw: 0x1000 * (k + 1) for k, kw in enumerate(keyword.values())}
    for absent in ((), ("albedo_low",), ("albedo",), ("halves_low_ptr", "halves_out_ptr"), ("rgba8_ptr", "weight_out_ptr", "stream_ptr")):
        kw = dict(values, params=prm, **{a: None for a in absent})
        capi.DeviceScene.upsample_device(scene, 3, 2, 7, 5, **kw)
        got = _one_call(recorder, "rr_upsample_albedo_records_device", names)
        assert _address(got["scene"]) == HANDLE and got["params"]._obj is prm
        assert [got[k].value for k in ("low_width", "low_height", "width", "height")] == [3, 2, 7, 5]
        for header_name, k in keyword.items():
            assert _address(got[header_name]) == (kw[k] or 0), f"{header_name} with {absent} absent"
    # with both planes None the call is the older symbol
    capi.DeviceScene.upsample_device(scene, 3, 2, 7, 5, **dict(values, params=prm, albedo_low=None, albedo=None))
    _one_call(recorder, "rr_upsample_records_device", _param_names(_header(), "rr_upsample_records_device"))


def test_host_form_passes_the_callers_arrays_in_the_headers_order(recorder, scene):
    names = _param_names(_header(), "rr_upsample_albedo_records")
    assert names == ["scene", "low_width", "low_height", "width", "height", "params", "low", "halves_low", "guide_low", "guide", "albedo_low", "albedo", "out",
                     "halves_out", "rgba8_out", "weight_out"]
    w, h, W, H = 3, 2, 6, 4
    rng = np.random.default_rng(5)
    prm = capi.rr_upsample_params()
    for with_low, with_full in ((True, True), (True, False), (False, True)):
        for with_halves in (True, False):
            a = dict(low=rng.random((w * h, 8), np.float32), halves_low=rng.random((w * h, 2, 8), np.float32) if with_halves else None,
                     guide_low=np.zeros(w * h, SURFACE_HIT_DTYPE), guide=np.zeros(W * H, SURFACE_HIT_DTYPE),
                     albedo_low=rng.random((w * h, 3), np.float32) if with_low else None, albedo=rng.random((W * H, 3), np.float32) if with_full else None)
            res = capi.DeviceScene.upsample(scene, w, h, W, H, params=prm, rgba8=True, **a)
            got = _one_call(recorder, "rr_upsample_albedo_records", names)
            what = f"low={with_low} full={with_full} halves={with_halves}"
            assert _address(got["scene"]) == HANDLE and got["params"]._obj is prm, what
            assert [got[k].value for k in ("low_width", "low_height", "width", "height")] == [w, h, W, H], what
            for k, v in a.items():       # the caller's own memory, no copy; NULL where the caller has none
                assert _address(got[k]) == (v.ctypes.data if v is not None else 0), f"{what}: {k}"
            for o, key in (("out", "records"), ("halves_out", "halves"), ("rgba8_out", "rgba"), ("weight_out", "weight")):
                r = res.get(key)
                assert _address(got[o]) == (r.ctypes.data if r is not None else 0), f"{what}: {o}"
    a.update(albedo_low=None, albedo=None)
    capi.DeviceScene.upsample(scene, w, h, W, H, params=prm, **a)
    _one_call(recorder, "rr_upsample_records", _param_names(_header(), "rr_upsample_records"))


def test_the_pipelines_refuse_unknown_options():
    from rustray_amd import renderer
    from rustray_amd.renderer import Raytracing
    rt = object.__new__(Raytracing)        # (the options are checked before anything of the object is looked at)
    for bad in ("centre", "diffuse", False, None, 1):
        with pytest.raises(ValueError, match="albedo"):
            rt.render_upsampled(albedo=bad)
        with pytest.raises(ValueError, match="albedo"):
            renderer.render_upsampled_torch(None, None, None, albedo=bad)
    for bad in (0, -1, 1.5, True, "2"):
        with pytest.raises(ValueError, match="full_albedo_samples"):
            rt.render_upsampled(albedo="mean", full_albedo_samples=bad)
        with pytest.raises(ValueError, match="full_albedo_samples"):
            renderer.render_upsampled_torch(None, None, None, full_albedo_samples=bad)
