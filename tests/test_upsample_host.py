"""The joint-bilateral upsampler of rr_upsample_records without a GPU: the host loop over rustray_amd/csrc/rr_upsample.h (the functions the
kernel applies per lane) under AddressSanitizer + UBSan against the numpy yardstick rustray_amd/upsample.py, bit for bit; the yardstick's
own properties and its quality against plain bilinear interpolation; what the entry points refuse before they touch a device; and the
binding's argument order against the header's parameter names."""
import ctypes as C
import inspect
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from rustray_amd import capi, upsample
from rustray_amd.flat import SURFACE_HIT_DTYPE
from rustray_amd.upsample import UpsampleParams, bilinear_records, upsample_records
from tests.denoise_cases import F, same_bits
from tests.helpers import ROOT, host_api_source
from tests.test_temporal_binding_host import HANDLE, _address, _header, _one_call, _param_names, recorder, scene  # noqa: F401 (fixtures)
from tests.upsample_cases import SHAPES, flat_guide, quality_case, random_case, records_of

NEW = ("rr_upsample_default_params", "rr_upsample_records_device", "rr_upsample_records")


@pytest.fixture(scope="module")
def host_loop(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("upsample") / "upsample_test")
    cmd = ["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-o", exe, os.path.join(ROOT, "tests", "native", "upsample_test.cpp")]
    subprocess.check_call(cmd)

    def run(tmp_path, w, h, W, H, low, halves, guide_low, guide, prm):
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(src, "wb") as fh:
            fh.write(struct.pack("<7If", w, h, W, H, halves is not None, prm.normal_power_log2, bool(prm.use_albedo), prm.sigma_depth))
            for a in (low, halves):
                if a is not None:
                    fh.write(np.ascontiguousarray(a, F).tobytes())
            fh.write(guide_low.tobytes())
            fh.write(guide.tobytes())
        out = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and "upsample test OK" in out.stdout, out.stdout + out.stderr
        raw = np.fromfile(dst, F)
        n, k = W * H, (24 if halves is not None else 8)
        assert raw.size == (k + 1) * n
        return dict(records=raw[:8 * n].reshape(n, 8), halves=raw[8 * n:k * n].reshape(n, 2, 8) if halves is not None else None, weight=raw[k * n:])
    return run


def _same(got, want, what):
    for key in ("records", "halves", "weight"):
        if want[key] is None:
            assert got[key] is None, (what, key)
            continue
        g, w = got[key].view(np.uint32), want[key].view(np.uint32)
        assert g.shape == w.shape and same_bits(g, w), f"{what}: {int((g != w).sum())} words of {key} differ"


def test_the_random_case_holds_what_it_promises():
    """5 ids, missed pixels in both guides, NaN and inf colours, a NaN normal on a hit, albedos of 0, 2^-10 and NaN."""
    low, halves, guide_low, guide = random_case(*SHAPES[0])
    assert np.isnan(low[:, 0:3]).any() and np.isinf(low[:, 0:3]).any() and (~np.isfinite(halves[:, :, 0:3]).all(-1).all(-1) & np.isfinite(low[:, 0:3]).all(-1)).any()
    for g in (guide_low, guide):
        hit = g["hit"] != 0
        assert set(np.unique(g["object_id"][hit])) == {1, 2, 3, 4, 5}
        assert (~hit).any() and hit.any()
        assert np.isnan(g["normal"][hit]).any()
        a = g["base_color"][hit][:, 0:3]
        assert (a == 0).any() and (a == F(2.0 ** -10)).any() and np.isnan(a).any()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_from_%dx%d" % s)
@pytest.mark.parametrize("power", (0, 5, 7))
def test_host_loop_equals_the_yardstick(host_loop, tmp_path, shape, power):
    W, H, w, h = shape
    low, halves, guide_low, guide = random_case(W, H, w, h)
    for use_halves in (True, False):
        for use_albedo in (True, False):
            prm = UpsampleParams(normal_power_log2=power, sigma_depth=0.05 if power else 0.3, use_albedo=use_albedo)
            hv = halves if use_halves else None
            _same(host_loop(tmp_path, w, h, W, H, low, hv, guide_low, guide, prm), upsample_records(low, hv, guide_low, guide, w, h, W, H, prm),
                  f"{W}x{H} <- {w}x{h} power {power} halves={use_halves} albedo={use_albedo}")


# ---- properties of the yardstick ------------------------------------------------------------------------------------------------
def test_equal_sizes_return_the_low_colour_where_the_id_matches():
    """w = W, h = H: u is x itself, so x0 = x and fx = 0: tap (0, 0) has b = 1 and the other three b = 0.  Without albedo and with power 0
    (cs = max(0, n_p . n_q) is still a factor, so the normals are kept at unit length with an exact dot product: the guides' own where the
    guides agree) the sum is 1 * c + 0 * c' and sum_w 1 + 0: the low colour's bits wherever the centre tap is taken."""
    W, H = 33, 9
    rng = np.random.default_rng(3)
    ids = (1 + (np.arange(W * H) // 7) % 3).astype(np.uint32)
    guide = flat_guide(W, H, ids=ids)
    ids_low = ids.copy()
    ids_low[rng.random(W * H) < 0.2] = 9
    guide_low = flat_guide(W, H, ids=ids_low)
    color = rng.random((W * H, 3)).astype(F) * F(3)
    low = records_of(color, guide_low)
    got = upsample_records(low, None, guide_low, guide, W, H, W, H, UpsampleParams(normal_power_log2=0, use_albedo=False))
    match = ids_low == ids
    assert match.any() and (~match).any()
    assert same_bits(got["records"][match, 0:3].view(np.uint32), color[match].view(np.uint32))
    assert (got["weight"][match] == 1).all()


@pytest.mark.parametrize("shape", SHAPES[:3] + ((64, 48, 32, 24),), ids=lambda s: "%dx%d_from_%dx%d" % s)
def test_a_constant_colour_comes_back_exactly_under_any_guide(shape):
    """Every tap holds the colour c: the guided sum is (sum wt * c) / (sum wt) and the fallback the same with b.  For c = 0.5, a power of
    two, every product wt * c is exact (a change of exponent; no weight here is small enough to underflow) and so is every partial sum of
    them, half the partial sum of the weights: the quotient is c exactly.  Every colour of the low frame is finite and one of a pixel's
    two tap columns and rows always lies inside the low frame with a positive b, so the fallback never answers with zeros here."""
    W, H, w, h = shape
    _, _, guide_low, guide = random_case(W, H, w, h)
    color = np.full((w * h, 3), 0.5, F)
    low = records_of(color, guide_low)
    halves = np.stack([low, low], axis=1)
    got = upsample_records(low, halves, guide_low, guide, w, h, W, H, UpsampleParams(use_albedo=False))
    assert (got["records"][:, 0:3] == F(0.5)).all() and (got["halves"][:, :, 0:3] == F(0.5)).all()


def _two_id_frame(W, H, w, h):
    def ids(Wk, Hk):
        y, x = np.mgrid[0:Hk, 0:Wk]
        return np.where((x.reshape(-1) + 0.5) / Wk > 0.3 + 0.4 * (y.reshape(-1) + 0.5) / Hk, 7, 3).astype(np.uint32)
    guide, guide_low = flat_guide(W, H, ids=ids(W, H)), flat_guide(w, h, ids=ids(w, h))
    color = np.repeat((guide_low["object_id"] == 7).astype(F)[:, None], 3, axis=1)
    return records_of(color, guide_low), guide_low, guide


def test_no_colour_crosses_an_id_edge():
    """Two ids with the colours 0 and 1, same normal and depth on both sides: only the id separates them.  A guided pixel (weight > 0)
    sums taps of its own id alone, all of one colour: it is 0 or 1 exactly, and it is its own id's colour."""
    W, H, w, h = 64, 48, 32, 24
    low, guide_low, guide = _two_id_frame(W, H, w, h)
    got = upsample_records(low, None, guide_low, guide, w, h, W, H, UpsampleParams(use_albedo=False))
    guided = got["weight"] > 0
    assert guided.sum() > 0.9 * W * H
    c = got["records"][guided, 0]
    assert np.isin(c, (0.0, 1.0)).all()
    assert np.array_equal(c == 1, guide["object_id"][guided] == 7)
    blurred = bilinear_records(low, None, guide, w, h, W, H)["records"][:, 0]
    assert ((blurred > 0) & (blurred < 1)).any()      # (what plain interpolation does at the same edge)


def test_the_weight_is_zero_exactly_where_no_tap_passes_the_skip_rule():
    """On a frame whose taken taps all weigh something -- scale 2 (fx and fy are 1/4 or 3/4: every b is positive), one unit normal and
    depths close enough that no weight underflows -- sum_w is 0 exactly where the skip rule leaves no tap.  The rule is evaluated here
    per pixel, in plain Python, from the header's text."""
    W, H, w, h = 36, 20, 18, 10
    low, guide_low, guide = _two_id_frame(W, H, w, h)
    low = low.copy()
    low[5, 0], low[40, 1] = np.nan, np.inf
    guide["object_id"][11::W] = 9              # a pole one full pixel wide: no low pixel saw it
    guide["object_id"][7 * W + 20:7 * W + 30] = 11
    got = upsample_records(low, None, guide_low, guide, w, h, W, H)
    x0, _ = upsample.position(W, w)
    y0, _ = upsample.position(H, h)
    fin = np.isfinite(low[:, 0:3]).all(-1)
    want = np.zeros(W * H, bool)
    for y in range(H):
        for x in range(W):
            for dy in (0, 1):
                for dx in (0, 1):
                    qx, qy = x0[x] + dx, y0[y] + dy
                    if 0 <= qx < w and 0 <= qy < h and fin[qy * w + qx] and guide_low["object_id"][qy * w + qx] == guide["object_id"][y * W + x]:
                        want[y * W + x] = True
    assert (~want).any() and want.any()
    assert np.array_equal(got["weight"] > 0, want) and (got["weight"][~want] == 0).all()


def test_the_guide_fields_of_out_are_the_full_guides():
    W, H, w, h = SHAPES[0]
    low, halves, guide_low, guide = random_case(W, H, w, h)
    got = upsample_records(low, halves, guide_low, guide, w, h, W, H)
    hit = guide["hit"] != 0
    for rec in (got["records"], got["halves"][:, 0], got["halves"][:, 1]):
        assert same_bits(rec[hit, 3].view(np.uint32), guide["distance"][hit].view(np.uint32))
        assert same_bits(rec[hit, 4:7].view(np.uint32), np.ascontiguousarray(guide["normal"][hit]).view(np.uint32))
        assert np.array_equal(rec[hit, 7].view(np.uint32), guide["object_id"][hit])
        # a miss: the record of a pixel all of whose rays missed -- depth +0, the device's 0 / 0 in the normal, id 0
        assert (rec[~hit, 3].view(np.uint32) == 0).all() and (rec[~hit, 7].view(np.uint32) == 0).all()
        assert (rec[~hit, 4:7].view(np.uint32) == 0xFFC00000).all()


def test_quality_against_plain_bilinear_interpolation():
    """64x48 <- 32x24, a textured albedo times a smooth shade per id (tests/upsample_cases.py: quality_case): the guided result is closer
    to the full-resolution truth than bilinear_records of the same low frame (this frame: printed below, recorded in DESIGN.md)."""
    truth, low, guide_low, guide = quality_case()
    mse = lambda rec: float(np.mean((rec[:, 0:3].astype(np.float64) - truth) ** 2))
    guided = mse(upsample_records(low, None, guide_low, guide, 32, 24, 64, 48)["records"])
    plain = mse(bilinear_records(low, None, guide, 32, 24, 64, 48)["records"])
    print(f"MSE guided {guided:.3e}, bilinear {plain:.3e}, ratio {plain / guided:.1f}")
    assert guided < plain


# ---- the entry points, without a device -----------------------------------------------------------------------------------------
def test_default_params():
    p = capi.upsample_default_params()
    assert C.sizeof(capi.rr_upsample_params) == 20 == p.struct_size
    d = UpsampleParams()
    assert (p.normal_power_log2, p.use_albedo, p.gamma_correction) == (d.normal_power_log2, 1, 0) == (5, 1, 0)
    assert p.sigma_depth == F(d.sigma_depth) == F(0.05)
    assert capi.lib().rr_upsample_default_params(None) == -1
    hdr = open(os.path.join(ROOT, "include", "rustray_hip.h")).read()
    body = re.search(r"typedef struct rr_upsample_params \{(.*?)\} rr_upsample_params;", hdr, re.S).group(1)
    assert re.findall(r"(\w+);", body) == [f[0] for f in capi.rr_upsample_params._fields_]


def test_refusals_without_a_device():
    """Every call below is refused on its arguments alone, before the scene is looked at: the made-up handle is never dereferenced."""
    L = capi.lib()
    w, h, W, H = 10, 6, 20, 12
    nl, n = w * h, W * H
    low, halves = np.full((nl, 8), 0.5, F), np.full((nl, 2, 8), 0.5, F)
    guide_low, guide = np.zeros(nl + 1, SURFACE_HIT_DTYPE), np.zeros(n + 1, SURFACE_HIT_DTYPE)
    out, hout = np.full((n + 4, 8), 7.0, F), np.full((n + 4, 2, 8), 7.0, F)
    rgba, wt = np.full((n + 4, 4), 0x5a, np.uint8), np.full(n + 4, 7.0, F)
    fake = C.c_void_p(0x1000)
    P = lambda a, off=0: C.c_void_p(a.ctypes.data + off)
    good = capi.upsample_default_params

    for name, dev in (("rr_upsample_records", False), ("rr_upsample_records_device", True)):
        fn = getattr(L, name)

        def call(scene=fake, lw=w, lh=h, fw=W, fh=H, prm=None, lo=P(low), hv=P(halves), gl=P(guide_low), gf=P(guide), o=P(out), ho=P(hout), rg=P(rgba), wo=P(wt),
                 null_prm=False):
            p = prm or good()
            args = [scene, lw, lh, fw, fh, None if null_prm else C.byref(p), lo, hv, gl, gf, o, ho, rg, wo]
            return fn(*(args + [None] if dev else args))

        err = lambda: L.rr_last_error()
        assert call(scene=None) == -1 and b"scene" in err()
        assert call(null_prm=True) == -1 and b"params" in err()
        for kw, word in ((dict(lo=None), b"low is NULL"), (dict(gl=None), b"guide_low is NULL"), (dict(gf=None), b"guide is NULL"), (dict(o=None), b"out is NULL")):
            assert call(**kw) == -1 and word in err(), (name, kw, err())
        assert call(fw=0) == -1 and call(fh=0) == -1 and b"frame size" in err()
        assert call(fw=65536) == -1 and call(fh=65536) == -1 and b"frame size" in err()
        assert call(lw=0) == -1 and call(lh=0) == -1 and b"low frame size" in err()
        assert call(lw=W + 1) == -1 and call(lh=H + 1) == -1 and b"low frame size" in err()
        for field, values in (("struct_size", (0, 16, 24)), ("normal_power_log2", (8, 0xffffffff)), ("sigma_depth", (0.0, -1.0, float("nan"), float("inf")))):
            for val in values:
                p = good()
                setattr(p, field, val)
                assert call(prm=p) == -1, (name, field, val)
                assert field.encode() in err(), (name, field, err())
        assert call(hv=None) == -1 and b"together" in err()
        assert call(ho=None) == -1 and b"together" in err()
        if dev:   # the alignment rules of the device form
            for kw in (dict(lo=P(low, 8)), dict(hv=P(halves, 4)), dict(gl=P(guide_low, 8)), dict(gf=P(guide, 4)), dict(o=P(out, 8)), dict(ho=P(hout, 4))):
                assert call(**kw) == -1 and b"16-byte aligned" in err(), (name, kw)
            assert call(rg=P(rgba, 1)) == -1 and call(wo=P(wt, 2)) == -1 and b"4-byte aligned" in err()
        # overlaps: nothing is in place
        assert call(o=P(low)) == -1 and b"out overlaps low" in err()
        assert call(o=P(guide, 128)) == -1 and b"out overlaps guide" in err()
        assert call(ho=P(halves)) == -1 and b"halves_out overlaps halves_low" in err()
        assert call(rg=P(guide_low)) == -1 and b"rgba8_out overlaps guide_low" in err()
        assert call(wo=P(out, 32 * n - 16)) == -1 and b"out overlaps weight_out" in err()
        assert call(ho=P(out, 64)) == -1 and b"out overlaps halves_out" in err()
        assert call(rg=P(wt), wo=P(wt)) == -1 and b"rgba8_out overlaps weight_out" in err()
        # more than 2^30 half records: the last refusal, so the made-up buffers lie 2^40 bytes apart and overlap nothing
        far = lambda k: C.c_void_p((k + 1) << 40)
        big = dict(lw=1, lh=1, fw=32768, fh=16385, lo=far(0), hv=far(1), gl=far(2), gf=far(3), o=far(4), ho=far(5), rg=far(6), wo=far(7))
        assert call(**big) == -2 and b"2^30" in err()
        assert call(**dict(big, wo=far(4))) == -1 and b"overlaps" in err()     # (an overlap is named before the size is)
    assert (out == 7.0).all() and (hout == 7.0).all() and (rgba == 0x5a).all() and (wt == 7.0).all()


def test_the_new_entry_points_are_guarded_and_bound():
    src = host_api_source()
    for name in NEW:
        assert re.search(r'^int ' + name + r'\([^{]*\) try \{', src, re.M), f"{name} is not a function-try-block"
        assert f'RR_GUARD_END("{name}")' in src
        assert name in capi.EXPORTS and hasattr(capi.lib(), name) and getattr(capi.lib(), name).argtypes is not None
    assert "rr_api_upsample.h" in capi.LIB_SOURCES and "rr_upsample.h" in capi.LIB_SOURCES
    mk = open(os.path.join(ROOT, "rustray_amd", "csrc", "Makefile")).read()
    assert "rr_api_upsample.h" in mk and "rr_upsample.h" in mk
    # rr_upsample.h is plain host logic: rr_denoise.h is its one include, and it makes no HIP call and copies nothing of that header
    text = open(os.path.join(ROOT, "rustray_amd", "csrc", "rr_upsample.h")).read()
    assert re.findall(r"#include\s+(\S+)", text) == ['"rr_denoise.h"']
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    assert not re.search(r"\bhip[A-Z]\w*\s*\(", code)
    for reused in ("denoise_is_finite", "denoise_demodulate", "denoise_remodulate", "DN_EPS", "DN_FLT_MAX"):
        assert reused in code and not re.search(r"(#define|float|bool)\s+" + reused + r"\b", code), reused
    for m in ("upsample", "upsample_device"):
        assert hasattr(capi.DeviceScene, m)
    from rustray_amd import renderer
    assert hasattr(renderer, "upsample_torch") and hasattr(renderer, "render_upsampled_torch")
    assert hasattr(renderer.Raytracing, "render_upsampled")


# ---- the binding's argument order against the header's parameter names -------------------------------------------------------------
def test_device_form_passes_every_argument_in_the_headers_order(recorder, scene):
    names = _param_names(_header(), "rr_upsample_records_device")
    assert names[:6] == ["scene", "low_width", "low_height", "width", "height", "params"] and names[-1] == "hip_stream"
    fn = capi.DeviceScene.upsample_device
    pointers = [p for p in inspect.signature(fn).parameters if p.endswith("_ptr")]
    header_name = lambda p: dict(rgba8_ptr="rgba8_out_dev", stream_ptr="hip_stream").get(p, p[:-4] + "_dev")
    assert sorted(header_name(p) for p in pointers) == sorted(names[6:])
    prm = capi.rr_upsample_params()
    values = {p: 0x1000 * (k + 1) for k, p in enumerate(pointers)}
    for absent in (None, "halves_low_ptr", "halves_out_ptr", "rgba8_ptr", "weight_out_ptr", "stream_ptr"):
        kw = dict(values, params=prm)
        if absent:
            kw[absent] = None
        fn(scene, 3, 2, 7, 5, **kw)
        got = _one_call(recorder, "rr_upsample_records_device", names)
        assert _address(got["scene"]) == HANDLE and got["params"]._obj is prm
        assert [got[k].value for k in ("low_width", "low_height", "width", "height")] == [3, 2, 7, 5]
        for p in pointers:
            assert _address(got[header_name(p)]) == (kw[p] or 0), f"{header_name(p)} with {absent} absent"


def test_host_form_passes_the_callers_arrays_and_the_results_in_the_headers_order(recorder, scene):
    names = _param_names(_header(), "rr_upsample_records")
    assert names == ["scene", "low_width", "low_height", "width", "height", "params", "low", "halves_low", "guide_low", "guide", "out", "halves_out", "rgba8_out",
                     "weight_out"]
    w, h, W, H = 3, 2, 6, 4
    rng = np.random.default_rng(5)
    prm = capi.rr_upsample_params()
    for with_halves in (True, False):
        for rgba8 in (False, True):
            for weight in (True, False):
                a = dict(low=rng.random((w * h, 8), np.float32), halves_low=rng.random((w * h, 2, 8), np.float32) if with_halves else None,
                         guide_low=np.zeros(w * h, SURFACE_HIT_DTYPE), guide=np.zeros(W * H, SURFACE_HIT_DTYPE))
                res = capi.DeviceScene.upsample(scene, w, h, W, H, params=prm, rgba8=rgba8, weight=weight, **a)
                got = _one_call(recorder, "rr_upsample_records", names)
                what = f"halves={with_halves} rgba8={rgba8} weight={weight}"
                assert _address(got["scene"]) == HANDLE and got["params"]._obj is prm, what
                assert [got[k].value for k in ("low_width", "low_height", "width", "height")] == [w, h, W, H], what
                for k, v in a.items():       # the caller's own memory, no copy; NULL where the caller has none
                    assert _address(got[k]) == (v.ctypes.data if v is not None else 0), f"{what}: {k}"
                for o, key, shape, dtype in (("out", "records", (W * H, 8), np.float32), ("halves_out", "halves", (W * H, 2, 8), np.float32),
                                             ("rgba8_out", "rgba", (W * H, 4), np.uint8), ("weight_out", "weight", (W * H,), np.float32)):
                    r = res.get(key)
                    present = dict(out=True, halves_out=with_halves, rgba8_out=rgba8, weight_out=weight)[o]
                    assert (r is not None) == present, f"{what}: {o}"
                    assert _address(got[o]) == (r.ctypes.data if present else 0), f"{what}: {o}"
                    if present:
                        assert r.shape == shape and r.dtype == dtype and r.flags.c_contiguous, f"{what}: {o}"
