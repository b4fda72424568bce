"""rr_denoise_records on the device at the ends of the float range and at the shapes the pass kernels' forms had not seen, every output
word against the numpy yardstick rustray_amd/denoise.py.

1: the range frames of tests/denoise_cases.py (subnormal and huge colours, negative colours, depths of both signs over the whole range,
zero, short, huge and flipped normals, zero and tiny variances, an albedo over the whole range, all of it at once next to NaN / inf
pixels) at 37x19, power 5 and 7, with and without halves: strictly bitwise but for the NaNs the arithmetic generates, which match as
NaNs: in `mixed`, and in the variances of `colour_range` with halves (tests/test_denoise_range_host.py says where the yardstick has
them); `colour_bands` is the colour range without them, and `demod_overflow` the input the header asks a caller to avoid; 2: five of
them at 130x70 in every form of the pass kernel, where subnormals, infs and weightless pixels go through LDS and sit at tile seams;
3: one column, one row, a lane and a row past a tile, exact tiles, and frames smaller than the lattice, on random_frame and `mixed`,
each form forced and automatic; 4: in place and the host form."""
import numpy as np
import pytest

from rustray_amd import denoise
from rustray_amd.denoise import DenoiseParams, atrous_denoise
from tests.denoise_cases import RANGE_KINDS, random_frame, range_frame
from tests.test_gpu_denoise import _check, _device_call, small_scene  # noqa: F401  (small_scene: the fixture)

pytestmark = pytest.mark.gpu

KINDS = RANGE_KINDS + ("colour_bands",)
WITH_ALBEDO = ("albedo_range", "mixed", "demod_overflow")
_want = {}


def _frame(kind, W, H):
    return random_frame(W, H) if kind == "random" else range_frame(W, H, kind)


def _yardstick(kind, W, H, use_halves, use_albedo, prm: DenoiseParams):
    """The yardstick's answer for a frame, computed once per case and left unchanged."""
    key = (kind, W, H, use_halves, use_albedo, prm.iterations, prm.normal_power_log2)
    if key not in _want:
        records, halves, albedo = _frame(kind, W, H)
        res = atrous_denoise(records, halves if use_halves else None, albedo if use_albedo else None, W, H, prm)
        res["rgba"] = denoise.frame_bytes_linear(res["records"][:, 0:3])
        _want[key] = res
    return _want[key]


def _run(ds, kind, W, H, use_halves, prm, what, **kw):
    use_albedo = kind in WITH_ALBEDO or kind == "random"
    got = _device_call(ds, W, H, use_halves, use_albedo, prm, frame=_frame(kind, W, H), **kw)
    # (tests/test_denoise_range_host.py: which kinds generate NaNs, and where)
    nan_equal = True if kind in ("mixed", "demod_overflow") else "variance" if kind == "colour_range" and use_halves else False
    _check(got, _yardstick(kind, W, H, use_halves, use_albedo, prm), what, nan_equal=nan_equal)
    return got


def _forms(hip):
    mixed = [hip.DENOISE_FORM_LATTICE, hip.DENOISE_FORM_GATHER, hip.DENOISE_FORM_TILE, hip.DENOISE_FORM_LATTICE, hip.DENOISE_FORM_GATHER, hip.DENOISE_FORM_LATTICE]
    return (("gather", [hip.DENOISE_FORM_GATHER] * 6), ("tile", [hip.DENOISE_FORM_TILE] * 6), ("lattice", [hip.DENOISE_FORM_LATTICE] * 6), ("mixed forms", mixed))


# ---- 1: every kind at 37x19 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_halves", (True, False))
@pytest.mark.parametrize("power", (5, 7))
@pytest.mark.parametrize("kind", KINDS)
def test_every_word_equals_the_yardstick_over_the_float_range(small_scene, kind, power, use_halves):  # noqa: F811
    prm = DenoiseParams(iterations=6, normal_power_log2=power)
    _run(small_scene, kind, 37, 19, use_halves, prm, f"{kind} 37x19 power {power} halves={use_halves}")


@pytest.mark.parametrize("use_halves", (True, False))
@pytest.mark.parametrize("W,H,iterations", ((37, 19, 1), (37, 19, 6), (130, 70, 1), (130, 70, 6)))
def test_where_demodulation_overflows(small_scene, W, H, iterations, use_halves):  # noqa: F811
    """The input the header asks a caller to avoid: an inf working colour that is a tap, and a NaN variance seed (both halves overflow:
    lum(inf) - lum(inf)) that is a tap of the 3x3 prefilter all the same -- k_denoise_prepare's "no tap" mark in LDS is a negative seed,
    and a NaN is not one.  One pass: most variances are still numbers; six: the infs and NaNs have gone through every form."""
    _run(small_scene, "demod_overflow", W, H, use_halves, DenoiseParams(iterations=iterations), f"demod_overflow {W}x{H} x{iterations} halves={use_halves}")


# ---- 2: through LDS and across tile seams ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("colour_range", "colour_bands", "normal_zero", "depth_range", "mixed"))
def test_every_form_of_the_pass_kernel_over_the_float_range(small_scene, hip, kind):  # noqa: F811
    prm = DenoiseParams(iterations=6)
    try:
        for name, forms in _forms(hip):
            hip.denoise_forms(forms)
            _run(small_scene, kind, 130, 70, True, prm, f"{kind} 130x70, {name}")
    finally:
        hip.denoise_forms(None)


# ---- 3: shapes the forms have not seen ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("random", "mixed"))
@pytest.mark.parametrize("W,H", ((1, 70), (70, 1), (33, 9), (64, 16)))
def test_thin_and_exact_frames_in_every_form(small_scene, hip, W, H, kind):  # noqa: F811
    """1x70 and 70x1: one column, one row (every horizontal or vertical tap outside); 33x9: one lane and one row past a 32x8 tile; 64x16:
    exact tiles, no partial workgroup."""
    prm = DenoiseParams(iterations=6)
    try:
        for name, forms in _forms(hip)[:3] + (("automatic", None),):
            hip.denoise_forms(forms)
            _run(small_scene, kind, W, H, True, prm, f"{kind} {W}x{H}, {name}")
    finally:
        hip.denoise_forms(None)


@pytest.mark.parametrize("kind", ("random", "mixed"))
@pytest.mark.parametrize("W,H", ((3, 2), (5, 5)))
def test_frames_smaller_than_the_lattice(small_scene, hip, W, H, kind):  # noqa: F811
    """Every pass from step 2 on as one tile per residue class of the step's sub-lattice, on a frame where most classes of the large
    steps hold no pixel at all."""
    prm = DenoiseParams(iterations=6)
    try:
        hip.denoise_forms([hip.DENOISE_FORM_LATTICE] * 6)
        _run(small_scene, kind, W, H, True, prm, f"{kind} {W}x{H}, lattice")
    finally:
        hip.denoise_forms(None)


# ---- 4: in place, and the host form ------------------------------------------------------------------------------------------------
def test_in_place_and_host_form_on_the_mixed_frame(small_scene):  # noqa: F811
    W, H = 37, 19
    prm = DenoiseParams(iterations=6)
    records, halves, albedo = range_frame(W, H, "mixed")
    dev = _run(small_scene, "mixed", W, H, True, prm, "mixed 37x19")
    same = _run(small_scene, "mixed", W, H, True, prm, "mixed 37x19 in place", in_place=True)
    host = small_scene.denoise_records(W, H, records, halves, albedo, prm, rgba8=True)
    # one device, one code: the same words, NaNs included
    for a, b in zip(dev, same):
        assert np.array_equal(a, b)
    assert np.array_equal(host["records"].view(np.uint32), dev[0]) and np.array_equal(host["variance"].view(np.uint32), dev[1]) and np.array_equal(host["rgba"], dev[2])
