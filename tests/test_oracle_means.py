"""The oracle's float64 side outputs (render(..., want_means=True, samples_used=k)) and the quantisation band of
tests/helpers.py that judges device pixels against them.  Host only: no GPU.

The band is only as good as the means under it: these tests pin that the means leave the oracle's own outputs bit
for bit as they were, that they describe the frame the oracle rendered (channel order, window, divisor), that a
preview's means are those of the first k samples, and that the band rejects errors ±1 LSB cannot see."""
import copy

import numpy as np
import pytest

from rustray_amd.flat import make_config
from tests.helpers import (BAND_ARG_SLACK, BAND_EPS_ABS, BAND_EPS_REL, D6_CLAMP, U32, as_u8, band_bytes, band_check,
                           band_stats, camera_for, compare_frames, depth_check, load_scene, normal_check)

CASES = [  # scene, w, h, config
    ("spheres", 40, 32, dict(samples=4, monte_carlo=True, seed=5)),
    ("earth_room", 40, 24, dict(samples=3, monte_carlo=True, seed=2, gamma_correction=True)),
    ("spheres_room", 40, 24, dict(samples=3, monte_carlo=True, seed=3, fog_density=0.02, fog_color=(0.2, 0.3, 0.5))),
    ("monkey", 40, 30, dict(samples=4, monte_carlo=True, seed=7, aperture_size=6.0, focal_length=8.0)),   # depth of field
    ("kbert_room", 40, 24, dict(samples=2, monte_carlo=True, seed=8, gamma_correction=True, max_recursion=3)),
]
KEYS = ("rgba", "depth", "normal", "object_id")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _render(oracle, name, w, h, kw, **opts):
    fs = load_scene(name)
    cam = camera_for(fs, w, h).c_struct()
    return oracle.render(fs.c_struct(), cam, make_config(**kw), n_threads=8, **opts)


def _own_band(ref, n, eps_rel=BAND_EPS_REL):
    """The oracle's bytes against its own means, with its f32 summation bound (n - 1)u|m| added to the band."""
    return band_stats(ref["rgba"][..., :3], ref["rgba"][..., :3], ref["mean_rgb"], ref["max_abs_rgb"],
                      ref["mean_gamma"][..., None], eps_rel + (n - 1) * U32, BAND_EPS_ABS)


@pytest.mark.parametrize("name,w,h,kw", CASES, ids=[c[0] for c in CASES])
def test_means_leave_every_output_bit_identical(oracle, name, w, h, kw):
    plain = _render(oracle, name, w, h, kw)
    means = _render(oracle, name, w, h, kw, want_means=True)
    for k in KEYS:
        assert np.array_equal(_bits(plain[k]), _bits(means[k])), k
    assert means["mean_rgb"].shape == (h, w, 3) and means["mean_rgb"].dtype == np.float64
    assert means["mean_depth"].shape == (h, w) and means["mean_normal"].shape == (h, w, 3)
    assert bool(means["mean_gamma"].all()) == bool(kw.get("gamma_correction", False))
    assert np.isfinite(means["mean_rgb"]).all() and (means["max_abs_rgb"] >= np.abs(means["mean_rgb"]) - 1e-12).all()


@pytest.mark.parametrize("name,w,h,kw", CASES, ids=[c[0] for c in CASES])
def test_oracle_bytes_lie_in_the_band_of_its_own_means(oracle, name, w, h, kw):
    ref = _render(oracle, name, w, h, kw, want_means=True)
    n = kw["samples"]
    res = _own_band(ref, n)
    assert res["n_rgb_outside_band"] == 0 and res["n_rgb_checked"] == w * h * 3, res
    assert (ref["mean_rgb"] > 0.02).sum() > w * h // 8      # lit: the band is judged on real colours, not on black
    d = depth_check(ref["depth"], ref["depth"], ref["mean_depth"], abs_err=0.0, rel_err=(n + 1) * U32)
    assert d["n_depth_outside"] == 0, d
    nr = normal_check(ref["normal"], ref["mean_normal"], term_err=(n + 1) * U32)
    assert nr["n_normal_outside"] == 0 and nr["n_normal_skipped"] < w * h, nr
    # the oracle's f32 mean, min(., 1), is the float64 mean within its summation bound: channel order and divisor
    f32 = np.minimum(ref["mean_rgb"], 1.0)
    assert np.allclose(ref["rgba"][..., :3] / 255.0, f32 if not kw.get("gamma_correction") else f32 ** (1 / 2.2), atol=1.5 / 255)


def test_window_means_land_on_their_pixels(oracle):
    name, w, h, kw = CASES[2]
    full = _render(oracle, name, w, h, kw, want_means=True)
    win = (7, 5, 29, 19)
    part = _render(oracle, name, w, h, kw, want_means=True, window=win)
    x0, y0, x1, y1 = win
    for k in ("mean_rgb", "mean_depth", "mean_normal", "max_abs_rgb"):
        assert np.array_equal(part[k][y0:y1, x0:x1], full[k][y0:y1, x0:x1]), k
        outside = part[k].copy()
        outside[y0:y1, x0:x1] = 0
        assert not outside.any(), k


def test_many_samples_bytes_lie_in_the_band_of_their_means(oracle):
    """4096 samples: the oracle's f32 sum drifts by up to (n - 1)u = 2.4e-4 relative; the band plus that bound holds it."""
    fs = load_scene("spheres")
    cam = camera_for(fs, 8, 6).c_struct()
    n = 4096
    ref = oracle.render(fs.c_struct(), cam, make_config(samples=n, monte_carlo=True, seed=5), n_threads=8, want_means=True)
    res = _own_band(ref, n)
    assert res["n_rgb_outside_band"] == 0 and res["n_rgb_checked"] == 8 * 6 * 3, res
    assert depth_check(ref["depth"], ref["depth"], ref["mean_depth"], abs_err=0.0, rel_err=(n + 1) * U32)["n_depth_outside"] == 0


@pytest.mark.parametrize("name", ["spheres_room", "monkey"])
def test_samples_used_renders_the_first_k_samples_of_the_frame(oracle, name):
    """N = 6 and k = 3, 4, 5 share cell_size 4: with the caller's table the first k samples of the 6-sample frame are
    the k-sample frame over the table's first k cells, bit for bit, means included."""
    fs = load_scene(name)
    cam = camera_for(fs, 24, 16).c_struct()
    N = 6
    T, cs = oracle.sample_table(N)
    assert cs == 4 and all(oracle.sample_table(k)[1] == 4 for k in (3, 4, 5))
    kw = dict(monte_carlo=True, seed=11, aperture_size=6.0, focal_length=8.0) if name == "monkey" else dict(monte_carlo=True, seed=11)
    whole = oracle.render(fs.c_struct(), cam, make_config(samples=N, **kw), sample_xy=T, n_threads=8, want_means=True)
    same = oracle.render(fs.c_struct(), cam, make_config(samples=N, **kw), sample_xy=T, n_threads=8, want_means=True, samples_used=N)
    for k in KEYS + ("mean_rgb", "mean_depth", "mean_normal", "max_abs_rgb"):
        assert np.array_equal(_bits(whole[k]), _bits(same[k])), k
    for k in (3, 4, 5):
        part = oracle.render(fs.c_struct(), cam, make_config(samples=N, **kw), sample_xy=T, n_threads=8, want_means=True, samples_used=k)
        direct = oracle.render(fs.c_struct(), cam, make_config(samples=k, **kw), sample_xy=T[:k], n_threads=8, want_means=True)
        for key in KEYS + ("mean_rgb", "mean_depth", "mean_normal", "max_abs_rgb"):
            assert np.array_equal(_bits(part[key]), _bits(direct[key])), (k, key)
        assert not np.array_equal(part["rgba"], whole["rgba"]), k
    # without a caller's table, samples_used takes the N-sample frame's own table
    a = oracle.render(fs.c_struct(), cam, make_config(samples=N, **kw), n_threads=8, samples_used=4)
    b = oracle.render(fs.c_struct(), cam, make_config(samples=4, **kw), sample_xy=T[:4], n_threads=8)
    assert np.array_equal(a["rgba"], b["rgba"])
    for bad in (0, N + 1, -1):
        with pytest.raises(ValueError):
            oracle.render(fs.c_struct(), cam, make_config(samples=N, **kw), n_threads=2, samples_used=bad)


def _lost_sample_case(oracle):
    fs = load_scene("spheres")
    cam = camera_for(fs, 48, 40).c_struct()
    N = 256
    cfg = make_config(samples=N, monte_carlo=True, seed=3)
    ref = oracle.render(fs.c_struct(), cam, cfg, n_threads=8, want_means=True)
    short = oracle.render(fs.c_struct(), cam, cfg, n_threads=8, want_means=True, samples_used=N - 1)
    return ref, short, N


def test_the_band_sees_a_lost_sample_and_a_quarter_lsb_bias_that_one_lsb_passes(oracle):
    """At 256 spp the frame a "one sample's terms lost" bug gives, q(m'(N - 1)/N) with m' the mean of the first N - 1
    samples, is within ±1 LSB of the oracle everywhere; the band rejects it in a large share of the lit channels.  So
    does a flat +0.25 LSB bias on the argument of as_u8."""
    ref, short, N = _lost_sample_case(oracle)
    lit = (ref["mean_rgb"] > 4 / 255) & (ref["mean_rgb"] < 250 / 255)
    assert lit.sum() > 400
    lost = ref.copy()
    lost_rgb = as_u8(255.0 * np.minimum(short["mean_rgb"] * (N - 1) / N, 1.0))
    lost["rgba"] = np.concatenate([lost_rgb.astype(np.uint8), ref["rgba"][..., 3:]], axis=-1)
    biased = ref.copy()
    bias_rgb = as_u8(255.0 * np.minimum(ref["mean_rgb"], 1.0) + 0.25)
    biased["rgba"] = np.concatenate([bias_rgb.astype(np.uint8), ref["rgba"][..., 3:]], axis=-1)
    # a channel moved by s LSB leaves its byte with probability s: the lost sample moves it by 255m/N LSB
    expected = {"lost": float((255.0 * ref["mean_rgb"] / N)[lit].sum()), "biased": 0.25 * float(lit.sum())}
    for what, bad in (("lost", lost), ("biased", biased)):
        res = compare_frames(bad, ref)
        assert res["n_rgb_over"] == 0, res                      # the ±1 LSB bar passes it ...
        miss = band_check(bad["rgba"][..., :3], ref["rgba"][..., :3], ref["mean_rgb"], ref["max_abs_rgb"])
        n_lit_miss = int((miss_mask(bad["rgba"][..., :3], ref) & lit).sum())
        assert res["n_rgb_outside_band"] == miss["n_rgb_outside_band"] > 0
        assert n_lit_miss > 0.6 * expected[what] and n_lit_miss > 0.1 * lit.sum(), (what, n_lit_miss, expected[what], int(lit.sum()))
    # and the frame made from the true means passes
    exact = ref.copy()
    exact["rgba"] = np.concatenate([as_u8(255.0 * np.minimum(ref["mean_rgb"], 1.0)).astype(np.uint8), ref["rgba"][..., 3:]], axis=-1)
    assert compare_frames(exact, ref)["n_rgb_outside_band"] == 0


def miss_mask(got_u8, ref):
    lo, hi = band_bytes(ref["mean_rgb"], ref["mean_gamma"][..., None])
    b = got_u8.astype(np.int32)
    return (b < lo) | (b > hi)


def _one(m, byte, gamma=False, ref_byte=None, max_abs=None, **kw):
    m = np.array([m], np.float64)
    return band_check(np.array([byte]), np.array([byte if ref_byte is None else ref_byte]), m,
                      np.array([abs(m[0]) if max_abs is None else max_abs]), gamma, **kw)


def test_band_by_hand():
    # a mean on a byte boundary admits both neighbours; just inside a byte admits that byte alone
    for b in (1, 77, 128, 254):
        m = b / 255.0
        assert band_bytes(m) == (b - 1, b)
        assert band_bytes(m + 1e-4) == (b, b) and band_bytes(m - 1e-4) == (b - 1, b - 1)
        assert _one(m, b)["n_rgb_outside_band"] == 0 and _one(m, b - 1)["n_rgb_outside_band"] == 0
        assert _one(m, b + 1)["n_rgb_outside_band"] == 1 and _one(m, b - 2)["n_rgb_outside_band"] == 1
    # the slack: 1e-3 LSB on the argument of as_u8, and e = 1e-5|m| + 2^-20 on the mean
    b = 128
    e = BAND_EPS_REL * b / 255 + BAND_EPS_ABS
    assert band_bytes(b / 255 + e + 0.5 * BAND_ARG_SLACK / 255) == (b - 1, b)
    assert band_bytes(b / 255 + e + 2.0 * BAND_ARG_SLACK / 255) == (b, b)
    # saturation: m >= 1 is 255 whatever its size; m just below 1 admits 254 and 255
    assert band_bytes(1.0) == (254, 255) and band_bytes(3.0) == (255, 255) and band_bytes(30000.0) == (255, 255)
    assert _one(5.0, 254)["n_rgb_outside_band"] == 1 and _one(5.0, 255)["n_rgb_outside_band"] == 0
    # m < 0 and m = 0 are black; a mean a hair above 0 still is
    assert band_bytes(-0.5) == (0, 0) and band_bytes(0.0) == (0, 0) and band_bytes(1e-7) == (0, 0)
    assert _one(-0.5, 1)["n_rgb_outside_band"] == 1
    # gamma near 0: pow(., 1/2.2) is steep, 255 * (1e-6)^(1/2.2) = 0.46 is still 0; the first byte starts at (1/255)^2.2
    assert band_bytes(1e-6, True) == (0, 0) and band_bytes(0.0, True) == (0, 0) and band_bytes(-1.0, True) == (0, 0)
    # there the absolute term matters: 2^-20 is 19 % of (1/255)^2.2 = 5.1e-6
    g1 = (1 / 255) ** 2.2
    assert band_bytes(g1 * 1.3, True) == (1, 1) and band_bytes(g1 * 0.7, True) == (0, 0) and band_bytes(g1, True) == (0, 1)
    assert band_bytes(0.5, True) == (as_u8(255 * 0.5 ** (1 / 2.2)),) * 2
    assert band_bytes(1.0, True) == (254, 255) and band_bytes(2.0, True) == (255, 255)
    # non-finite means must give the oracle's own byte (D6 flags: NaN or +inf -> 255, -inf -> 0)
    for m, ref_b in ((np.nan, 255), (np.inf, 255), (-np.inf, 0)):
        ok = _one(m, ref_b, ref_byte=ref_b, max_abs=np.inf)
        assert ok["n_rgb_outside_band"] == 0 and ok["n_rgb_nonfinite"] == 1 and ok["n_rgb_checked"] == 0
        assert _one(m, 128, ref_byte=ref_b, max_abs=np.inf)["n_rgb_outside_band"] == 1
    # a channel with a sample beyond the D6 clamp is excluded and counted, whatever its byte
    r = _one(0.3, 200, max_abs=2 * D6_CLAMP)
    assert r["n_rgb_outside_band"] == 0 and r["n_rgb_d6_excluded"] == 1 and r["n_rgb_checked"] == 0
    # the reported scale: the byte one above q(m) needs e reaching the next boundary
    m = 100.4 / 255
    r = _one(m, 101)
    assert r["n_rgb_outside_band"] == 1 and 0.5 < r["band_worst_miss_lsb"] < 0.7
    need = (101 - BAND_ARG_SLACK) / 255 - m
    assert r["band_eps_scale"] == pytest.approx(need / (BAND_EPS_REL * m + BAND_EPS_ABS), rel=1e-9)
    assert _one(m, 100)["band_eps_scale"] == 0.0
    # never wider than the ceiling
    with pytest.raises(AssertionError):
        _one(0.5, 128, eps_rel=2e-4)
    with pytest.raises(AssertionError):
        _one(0.5, 128, eps_abs=2.0 ** -15)


def test_depth_and_normal_bounds_by_hand():
    m = np.array([1.0, 600.0, np.nan])
    ok = depth_check(np.array([1.0 + 2.0 ** -18, 600.0 + 2.0 ** -17, np.nan], np.float32), np.array([0, 0, np.nan], np.float32), m)
    assert ok["n_depth_outside"] == 0
    bad = depth_check(np.array([1.0 + 2.0 ** -16, 600.0, 0.0], np.float32), np.array([0, 0, np.nan], np.float32), m)
    assert bad["n_depth_outside"] == 2
    # a NaN mean wants a NaN, of any sign or payload (the device writes a quiet NaN, x86 arithmetic a negative one)
    neg_nan = np.array([0xFFC00000], np.uint32).view(np.float32)
    assert depth_check(np.array([np.nan], np.float32), neg_nan, np.array([np.nan]))["n_depth_outside"] == 0
    assert depth_check(np.array([np.inf], np.float32), np.array([np.inf], np.float32), np.array([np.inf]))["n_depth_outside"] == 0
    assert depth_check(np.array([1e9], np.float32), np.array([np.inf], np.float32), np.array([np.inf]))["n_depth_outside"] == 1
    mn = np.array([[0.0, 0.5, 0.0], [0.0, 0.0, 1e-4], [0.6, 0.8, 0.0]])
    got = np.array([[0.0, 1.0, 0.0], [0.3, 0.3, 0.9], [0.6, 0.8 + 3e-7, 0.0]], np.float32)
    r = normal_check(got, mn)
    assert r["n_normal_skipped"] == 1 and r["n_normal_outside"] == 0
    got[2, 1] = np.float32(0.8 + 1e-5)
    assert normal_check(got, mn)["n_normal_outside"] == 1


def test_compare_frames_reports_the_band_only_with_means(oracle):
    name, w, h, kw = CASES[0]
    plain = _render(oracle, name, w, h, kw)
    means = _render(oracle, name, w, h, kw, want_means=True)
    assert "n_rgb_outside_band" not in compare_frames(plain, plain)
    res = compare_frames(plain, means)
    for k in ("n_rgb_outside_band", "n_rgb_in_band", "band_worst_miss_lsb", "n_depth_outside", "n_normal_outside", "n_normal_skipped"):
        assert k in res, k
    # the oracle's own 4-sample frame: its f32 drift at n = 4 is far inside the band
    assert res["n_rgb_outside_band"] == 0 and res["n_depth_outside"] == 0 and res["n_normal_outside"] == 0, res
    # a one-byte error where the band admits one byte only is caught
    lo, hi = band_bytes(means["mean_rgb"], False)
    y, x, c = np.argwhere((lo == hi) & (lo > 10) & (lo < 240))[0]
    wrong = copy.deepcopy(plain)
    wrong["rgba"][y, x, c] = lo[y, x, c] + 1
    assert compare_frames(wrong, means)["n_rgb_outside_band"] == 1
