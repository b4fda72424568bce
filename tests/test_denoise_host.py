"""The a-trous filter of rr_denoise_records without a GPU: the host loop over rustray_amd/csrc/rr_denoise.h (the functions the kernels apply
per lane) under AddressSanitizer + UBSan against the numpy yardstick rustray_amd/denoise.py, bit for bit; the yardstick's own properties
and its quality on a noisy frame; and what the entry points refuse before they touch a device."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from rustray_amd import capi, denoise
from rustray_amd.denoise import DenoiseParams, atrous_denoise
from tests.denoise_cases import F, pack, quality_frame, random_frame, same_bits
from tests.helpers import ROOT, host_api_source

NEW = ("rr_denoise_default_params", "rr_denoise_records_device", "rr_denoise_records")


@pytest.fixture(scope="module")
def host_loop(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("denoise") / "denoise_test")
    cmd = ["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-o", exe, os.path.join(ROOT, "tests", "native", "denoise_test.cpp")]
    subprocess.check_call(cmd)

    def run(tmp_path, W, H, records, halves, albedo, prm):
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(src, "wb") as fh:
            fh.write(struct.pack("<6I2f", W, H, halves is not None, albedo is not None, prm.iterations, prm.normal_power_log2, prm.sigma_depth, prm.sigma_luminance))
            for a in (records, halves, albedo):
                if a is not None:
                    fh.write(np.ascontiguousarray(a, F).tobytes())
        out = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and "denoise test OK" in out.stdout, out.stdout + out.stderr
        raw = np.fromfile(dst, F)
        assert raw.size == 9 * W * H
        return raw[:8 * W * H].reshape(W * H, 8), raw[8 * W * H:]
    return run


def _same_as_yardstick(got, want, what):
    rec, var = got
    assert same_bits(rec.view(np.uint32), want["records"].view(np.uint32)), f"{what}: {int((rec.view(np.uint32) != want['records'].view(np.uint32)).sum())} record words differ"
    assert same_bits(var.view(np.uint32), want["variance"].view(np.uint32)), f"{what}: variance differs"


def test_host_loop_equals_the_yardstick_on_the_quality_frame(host_loop, tmp_path):
    _, records, halves = quality_frame()
    prm = DenoiseParams()
    _same_as_yardstick(host_loop(tmp_path, 64, 48, records, halves, None, prm), atrous_denoise(records, halves, None, 64, 48, prm), "64x48 with halves")
    _same_as_yardstick(host_loop(tmp_path, 64, 48, records, None, None, prm), atrous_denoise(records, None, None, 64, 48, prm), "64x48 without halves")


@pytest.mark.parametrize("use_halves,use_albedo,prm", [
    (True, True, DenoiseParams()),
    (True, False, DenoiseParams(iterations=6, normal_power_log2=0, sigma_depth=0.3, sigma_luminance=1.5)),
    (False, True, DenoiseParams(iterations=3, normal_power_log2=7)),
    (False, False, DenoiseParams(iterations=1)),
])
def test_host_loop_equals_the_yardstick_on_a_random_frame(host_loop, tmp_path, use_halves, use_albedo, prm):
    """37x19, 5 ids, NaN / inf colours, non-finite halves, all-miss pixels (NaN normals, id 0), an albedo with zeros, 2^-10 and a NaN."""
    records, halves, albedo = random_frame(37, 19)
    assert np.isnan(records[:, 0]).any() and np.isinf(records[:, 2]).any() and np.isnan(records[:, 4]).any() and (albedo == 0).any()
    hv, al = (halves if use_halves else None), (albedo if use_albedo else None)
    _same_as_yardstick(host_loop(tmp_path, 37, 19, records, hv, al, prm), atrous_denoise(records, hv, al, 37, 19, prm), f"37x19 halves={use_halves} albedo={use_albedo}")


# ---- properties of the yardstick ------------------------------------------------------------------------------------------------
def _flat(W, H, color=(0.25, 0.5, 0.75), ident=4):
    n = W * H
    return pack(np.tile(np.array(color, F), (n, 1)), np.full(n, 3, F), np.tile(np.array([0, 0, 1], F), (n, 1)), np.full(n, ident, np.uint32))


def test_a_constant_frame_is_a_fixed_point():
    """Every tap holds the centre's colour: sum_c / sum_w is that colour again up to the rounding of the sums -- exactly, for a colour whose
    products with every weight and whose partial sums are exact (small dyadic rationals)."""
    rec = _flat(23, 17)
    halves = np.stack([rec, rec], axis=1)
    for hv in (None, halves):
        got = atrous_denoise(rec, hv, None, 23, 17, DenoiseParams(iterations=6))
        assert same_bits(got["records"].view(np.uint32), rec.view(np.uint32))
        assert (got["variance"] == 0).all()


def test_an_id_edge_is_never_crossed():
    W, H = 40, 24
    rec = _flat(W, H).copy()
    left = (np.arange(W * H) % W) < 17
    rec[left, 0:3], rec[left, 7] = F(8), np.uint32(9).view(F)      # same normal, same depth: only the id separates the halves
    got = atrous_denoise(rec, None, None, W, H, DenoiseParams(iterations=6))["records"]
    assert same_bits(got.view(np.uint32), rec.view(np.uint32))


def test_a_non_finite_pixel_passes_through_and_changes_no_neighbour():
    truth, records, halves = quality_frame()
    W, H = 64, 48
    bad = records.copy()
    at = 20 * W + 30
    bad[at, 0:3] = np.array([0x7fc01234, 0x7f800000, 0xff800000], np.uint32).view(F)   # a NaN with a payload, +inf, -inf
    got = atrous_denoise(bad, halves, None, W, H)
    assert same_bits(got["records"][at].view(np.uint32), bad[at].view(np.uint32)) and got["variance"][at] == 0
    assert np.isfinite(np.delete(got["records"][:, 0:3], at, axis=0)).all()
    # the neighbours are what they are when the pixel is simply no tap: the same frame with that pixel given an id of its own
    alone = records.copy()
    alone[at, 7] = np.uint32(0xabcdef).view(F)
    keep = np.arange(W * H) != at
    # (the variance prefilter also skips a non-finite tap, which an id does not: compare with the geometry-only filter, which has none)
    got_g = atrous_denoise(bad, None, None, W, H)["records"]
    want_g = atrous_denoise(alone, None, None, W, H)["records"]
    assert same_bits(got_g[keep].view(np.uint32), want_g[keep].view(np.uint32))


def test_one_iteration_on_one_pixel_returns_the_input():
    rec = pack(np.array([[0.3, 0.6, 0.9]], F), np.array([2.5], F), np.array([[0, 0.6, 0.8]], F), np.array([5], np.uint32))
    halves = np.stack([rec, rec], axis=1)
    halves[0, 0, 0:3] += F(0.125)
    halves[0, 1, 0:3] -= F(0.125)
    got = atrous_denoise(rec, halves, None, 1, 1, DenoiseParams(iterations=1, normal_power_log2=0))
    # the only tap is the centre: w = 9/64 * dot(n, n), and (w * c) / w is c for these values
    assert np.array_equal(got["records"][0, 3:], rec[0, 3:]) and np.allclose(got["records"][0, 0:3], rec[0, 0:3], rtol=2 ** -22, atol=0)
    n = rec[0, 4:7]
    w = F(0.375) * F(0.375) * ((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    want = np.array([(w * c) / w for c in rec[0, 0:3]], F)
    assert same_bits(got["records"][0, 0:3].view(np.uint32), want.view(np.uint32))
    rec1 = _flat(1, 1)
    assert same_bits(atrous_denoise(rec1, None, None, 1, 1, DenoiseParams(iterations=1))["records"].view(np.uint32), rec1.view(np.uint32))


def test_quality_on_the_noisy_frame():
    """64x48, halves = truth + N(0, 0.1), default parameters: the filtered frame is closer to the truth than the raw one by more than 2x
    (this frame: 0.0700 raw, 0.0098 with halves; 0.0647 geometry-only, which blurs the ramp: expected without a variance)."""
    truth, records, halves = quality_frame()
    rmse = lambda rec: float(np.sqrt(np.mean((rec[:, 0:3].astype(np.float64) - truth) ** 2)))
    raw = rmse(records)
    guided = rmse(atrous_denoise(records, halves, None, 64, 48)["records"])
    print(f"RMSE raw {raw:.4f}, denoised with halves {guided:.4f}, geometry-only {rmse(atrous_denoise(records, None, None, 64, 48)['records']):.4f}")
    assert 0.06 < raw < 0.08
    assert guided < raw * 0.5


# ---- the entry points, without a device -----------------------------------------------------------------------------------------
def test_default_params():
    p = capi.denoise_default_params()
    assert C.sizeof(capi.rr_denoise_params) == 24 == p.struct_size
    d = DenoiseParams()
    assert (p.iterations, p.normal_power_log2, p.gamma_correction) == (d.iterations, d.normal_power_log2, 0) == (5, 5, 0)
    assert p.sigma_depth == F(d.sigma_depth) == F(0.05) and p.sigma_luminance == F(d.sigma_luminance) == 4.0
    assert capi.lib().rr_denoise_default_params(None) == -1
    hdr = open(os.path.join(ROOT, "include", "rustray_hip.h")).read()
    assert "#define RR_MAX_DENOISE_ITERATIONS 6u" in hdr and denoise.MAX_ITERATIONS == 6


def test_refusals_without_a_device():
    """Every call below is refused on its arguments alone, before the scene is looked at: the made-up handle is never dereferenced."""
    L = capi.lib()
    W, H = 20, 12
    n = W * H
    rec = np.full((n, 8), 0.5, F)
    halves = np.full((n, 2, 8), 0.5, F)
    albedo = np.full((n + 4, 3), 0.5, F)
    out = np.full((n + 4, 8), 7.0, F)
    rgba = np.full((n + 4, 4), 0x5a, np.uint8)
    var = np.full(n + 4, 7.0, F)
    fake = C.c_void_p(0x1000)
    P = lambda a, off=0: C.c_void_p(a.ctypes.data + off)

    def good():
        return capi.denoise_default_params()

    for name, dev in (("rr_denoise_records", False), ("rr_denoise_records_device", True)):
        fn = getattr(L, name)

        def call(scene=fake, w=W, h=H, prm=None, r=P(rec), hv=P(halves), al=P(albedo), o=P(out), rg=P(rgba), v=P(var), null_prm=False):
            p = prm or good()
            args = [scene, w, h, None if null_prm else C.byref(p), r, hv, al, o, rg, v]
            return fn(*(args + [None] if dev else args))

        err = lambda: L.rr_last_error()
        assert call(scene=None) == -1 and b"scene" in err()
        assert call(null_prm=True) == -1 and b"params" in err()
        assert call(r=None) == -1 and b"records" in err()
        assert call(o=None) == -1 and b"out" in err()
        assert call(w=0) == -1 and call(h=0) == -1 and b"frame size" in err()
        assert call(w=65536, h=1) == -1 and call(w=1, h=65536) == -1
        assert call(w=32768, h=16385) == -2 and b"2^30" in err()
        for field, values in (("struct_size", (0, 20, 28)), ("iterations", (0, 7)), ("normal_power_log2", (8, 0xffffffff)),
                              ("sigma_depth", (0.0, -1.0, float("nan"), float("inf"))), ("sigma_luminance", (0.0, -0.5, float("nan"), float("inf")))):
            for val in values:
                p = good()
                setattr(p, field, val)
                assert call(prm=p) == -1, (name, field, val)
                assert field.encode() in err(), (name, field, err())
        # overlaps: only out == records, in place, is allowed (refused HERE for another reason or not at all -- see below)
        assert call(o=P(rec, 32)) == -1 and b"overlaps" in err()                   # out shifted by one record into records
        assert call(o=P(halves)) == -1 and b"out overlaps halves" in err()
        assert call(rg=P(rec)) == -1 and b"rgba8_out overlaps records" in err()
        assert call(v=P(albedo)) == -1 and b"variance_out overlaps albedo" in err()
        assert call(v=P(out, 32 * n - 4)) == -1 and b"out overlaps variance_out" in err()
        assert call(rg=P(var), v=P(var)) == -1 and b"rgba8_out overlaps variance_out" in err()
        if dev:   # the alignment rules of the device form
            assert call(r=P(rec, 8)) == -1 and b"16-byte aligned" in err()
            assert call(hv=P(halves, 4)) == -1 and b"16-byte aligned" in err()
            assert call(o=P(out, 8)) == -1 and b"16-byte aligned" in err()
            assert call(al=P(albedo, 2)) == -1 and b"4-byte aligned" in err()
            assert call(rg=P(rgba, 1)) == -1 and call(v=P(var, 2)) == -1 and b"4-byte aligned" in err()
    assert (out == 7.0).all() and (rgba == 0x5a).all() and (var == 7.0).all()


def test_the_new_entry_points_are_guarded_and_bound():
    src = host_api_source()
    for n in NEW:
        assert re.search(r'^int ' + n + r'\([^{]*\) try \{', src, re.M), f"{n} is not a function-try-block"
        assert f'RR_GUARD_END("{n}")' in src
        assert n in capi.EXPORTS and hasattr(capi.lib(), n) and getattr(capi.lib(), n).argtypes is not None
    assert "rr_api_denoise.h" in capi.LIB_SOURCES and "rr_denoise.h" in capi.LIB_SOURCES
    mk = open(os.path.join(ROOT, "rustray_amd", "csrc", "Makefile")).read()
    assert "rr_api_denoise.h" in mk and "rr_denoise.h" in mk
    # rr_denoise.h is plain host logic: no include of its own, no HIP call
    text = open(os.path.join(ROOT, "rustray_amd", "csrc", "rr_denoise.h")).read()
    assert "#include" not in text
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    assert not re.search(r"\bhip[A-Z]\w*\s*\(", code)
    for m in ("denoise_records", "denoise_records_device"):
        assert hasattr(capi.DeviceScene, m)
    from rustray_amd import renderer
    assert hasattr(renderer, "denoise_torch") and hasattr(renderer, "render_denoised_torch")
    assert hasattr(renderer.Raytracing, "denoise") and hasattr(renderer.Raytracing, "render_denoised")
