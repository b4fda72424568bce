"""The device's accumulator paths against the oracle's float64 means (run with -m gpu on an MI355X).

Hit geometry is pinned bit for bit elsewhere (test_gpu_trace_rays.py); what these frames pin is everything after the hit:
the 32-bit lane sums of fix_add, the segmented DPP merges, the 64-bit paths of colour terms of 2 and more and of root depths
beyond 512 units, and the divisor of k_resolve, also where a progressive preview reuses it with the samples finished so
far.  Each frame is judged by the quantisation band of tests/helpers.py on top of ±1 LSB."""
import numpy as np
import pytest

from rustray_amd.flat import make_config
from tests.helpers import INV_GAMMA, as_u8, assert_in_band, camera_for, compare_frames, load_scene
from tests.test_gpu_corners import _scaled_world
from tests.test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu


def _both(hip, oracle, fs, w, h, cfg, **ref_kw):
    cam = camera_for(fs, w, h).c_struct()
    with hip.DeviceScene(fs, 0) as ds:
        out = ds.render(cam, cfg)
    ref = oracle.render(fs.c_struct(), cam, cfg, want_means=True, n_threads=16, **ref_kw)
    return out, ref


def test_hundreds_of_samples_with_several_lights_and_reflections(hip, oracle):
    """300 samples of a 5-light room with reflective and textured surfaces: dozens of terms per sample reach each pixel,
    thousands per pixel in all.  A lost or doubled term of unit size moves a pixel by 0.85 LSB at this count: not
    necessarily past ±1 LSB, always out of the band."""
    fs = load_scene("earth_room")
    out, ref = _both(hip, oracle, fs, 24, 16, make_config(samples=300, monte_carlo=True, seed=12, max_recursion=4))
    r = assert_parity(out, ref, "earth_room 300 spp")
    assert r["n_rgb_checked"] == 24 * 16 * 3 and (ref["mean_rgb"] > 0.05).mean() > 0.5, r


def test_colour_terms_of_two_and_more_under_pixel_means_below_one(hip, oracle):
    """Lights four times as bright, with Monte Carlo jitter: many samples carry a colour component beyond 2 (a hit's lane sum
    then takes accum_merged's 64-bit path) while their pixel's mean stays below 1, where the byte sees every error."""
    fs = load_scene("spheres_room")
    for l in fs.lights:
        l.intensity = float(l.intensity) * 4.0
    out, ref = _both(hip, oracle, fs, 48, 32, make_config(samples=32, monte_carlo=True, seed=4))
    wide = (ref["max_abs_rgb"] > 2.0) & (ref["mean_rgb"] < 1.0)
    assert wide.sum() >= 100, int(wide.sum())
    assert (ref["max_abs_rgb"] > 32768.0).sum() == 0        # none excluded: every channel is judged
    r = assert_parity(out, ref, "bright lights")
    assert r["n_rgb_d6_excluded"] == 0


def _per_sample_depths(oracle, fs, cam, cfg):
    """The root depth of every sample: differences of the means over the first k samples (samples_used = k)."""
    n = cfg.samples
    prefix = [np.zeros((cam.height, cam.width))]
    for k in range(1, n + 1):
        prefix.append(oracle.render(fs.c_struct(), cam, cfg, n_threads=16, want_means=True, samples_used=k)["mean_depth"] * k)
    return np.stack([prefix[k] - prefix[k - 1] for k in range(1, n + 1)], axis=-1)


def test_far_depth_with_pixels_mixing_terms_below_and_beyond_512_units(hip, oracle):
    """spheres_room 40 times larger: root hits from 240 to 850 units, so the spheres' silhouettes against the walls mix
    depth terms of the 32-bit lane sums with 64-bit ones (accum_depth_wide_merged) inside one pixel.  Depth within half a
    2^-16 step of the float64 mean everywhere."""
    far = _scaled_world(load_scene("spheres_room"), 40.0)
    cfg = make_config(samples=8, monte_carlo=True, seed=6, max_recursion=2)
    out, ref = _both(hip, oracle, far, 40, 24, cfg)
    d = _per_sample_depths(oracle, far, camera_for(far, 40, 24).c_struct(), cfg)
    near_t, far_t = ((d > 0) & (d < 512)).any(-1), (d >= 512).any(-1)
    assert (near_t & ~far_t).sum() > 20 and (far_t & ~near_t).sum() > 20
    assert (near_t & far_t).sum() >= 5, int((near_t & far_t).sum())       # the silhouettes
    r = assert_parity(out, ref, "far")
    assert r["n_depth_outside"] == 0 and r["depth_scale"] <= 1.0


def test_progressive_previews_are_the_oracles_first_k_samples(hip, oracle):
    """rr_render_progressive: each preview is the frame resolved over the k sample slices finished so far, i.e. the oracle's
    frame of samples 0..k-1 of the same N-sample frame (samples_used = k), under gamma.  Object ids are exempt: they are final
    only after the last batch (include/rustray_hip.h)."""
    fs = load_scene("spheres_room")
    w, h, n = 64, 40, 12
    cam = camera_for(fs, w, h).c_struct()
    cfg = make_config(samples=n, monte_carlo=True, seed=9, gamma_correction=True)
    previews = []

    def on_pass(out, done, total):
        previews.append((done // (w * h), {k: v.copy() for k, v in out.items()}))
        return False
    with hip.DeviceScene(fs, 0) as ds:
        final = ds.render_progressive(cam, cfg, on_pass, min_passes=4)
    assert len(previews) >= 2 and all(0 < k < n for k, _ in previews)
    for k, got in previews + [(n, final)]:
        ref = oracle.render(fs.c_struct(), cam, cfg, n_threads=16, want_means=True, samples_used=k)
        got = dict(got)
        if k < n:
            got.pop("object_id")
        r = compare_frames(got, ref)
        assert r["alpha_ok"] and r["n_rgb_over"] == 0 and r["nan_mismatch"] == 0, (k, r)
        assert r["max_depth_rel"] < 1e-4 and r["max_normal_abs"] < 1e-4, (k, r)
        assert_in_band(r, f"preview after {k} of {n} samples")
    # the last preview as it would be resolved with the whole frame's divisor n instead of k: the band rejects it
    k0, first = previews[-1]
    ref0 = oracle.render(fs.c_struct(), cam, cfg, n_threads=16, want_means=True, samples_used=k0)
    g = np.clip(ref0["mean_rgb"] * k0 / n, 0.0, 1.0) ** INV_GAMMA
    wrong = dict(first, rgba=np.concatenate([as_u8(255.0 * g).astype(np.uint8), first["rgba"][..., 3:]], axis=-1))
    assert compare_frames({"rgba": wrong["rgba"]}, ref0)["n_rgb_outside_band"] > 0
