"""atrous_denoise_split (rustray_amd/denoise.py), the yardstick of rr_denoise_split_records, without a GPU: its two identities against
atrous_denoise on the frames of tests/denoise_cases.py, bit for bit except for the sign of a zero; a pixel whose record colour is not
finite keeps its colour; and the four new entry points are declared, exported, bound and guarded."""
import os
import re

import numpy as np
import pytest

from rustray_amd import capi
from rustray_amd.denoise import DenoiseParams, atrous_denoise, atrous_denoise_split
from tests.denoise_cases import quality_frame, random_frame
from tests.helpers import ROOT, host_api_source

F = np.float32


def _frames():
    _, rec, hv = quality_frame()
    yield "quality", 64, 48, rec, hv, np.full((64 * 48, 3), 0.5, F)
    for name, (W, H, bad) in dict(random_bad=(23, 17, True), random_clean=(16, 9, False)).items():
        rec, hv, al = random_frame(W, H, bad=bad)
        yield name, W, H, rec, hv, al


FRAMES = {f[0]: f[1:] for f in _frames()}


def same_but_zero_sign(got, want):
    """Two float32 arrays word by word: the same bits, or zeros of either sign on both sides."""
    g, w = np.ascontiguousarray(got, F).view(np.uint32), np.ascontiguousarray(want, F).view(np.uint32)
    both_zero = ((g << 1) == 0) & ((w << 1) == 0)
    return g.shape == w.shape and bool(((g == w) | both_zero).all())


@pytest.mark.parametrize("name", sorted(FRAMES))
@pytest.mark.parametrize("with_halves", (True, False))
def test_zero_diffuse_is_the_plain_filter(name, with_halves):
    W, H, rec, hv, al = FRAMES[name]
    n = W * H
    hv = hv if with_halves else None
    want = atrous_denoise(rec, hv, None, W, H)["records"]
    got = atrous_denoise_split(rec, hv, np.zeros((n, 3), F), np.zeros((n, 2, 3), F) if with_halves else None, al, W, H)["records"]
    assert same_but_zero_sign(got, want)


@pytest.mark.parametrize("name", sorted(FRAMES))
@pytest.mark.parametrize("with_halves", (True, False))
def test_all_diffuse_is_the_filter_with_the_albedo(name, with_halves):
    W, H, rec, hv, al = FRAMES[name]
    hv = hv if with_halves else None
    want = atrous_denoise(rec, hv, al, W, H)["records"]
    got = atrous_denoise_split(rec, hv, rec[:, 0:3], hv[:, :, 0:3] if with_halves else None, al, W, H)["records"]
    assert same_but_zero_sign(got, want)


def test_a_nonfinite_pixel_keeps_its_colour_and_the_rest_is_a_sum():
    W, H, rec, hv, al = FRAMES["random_bad"]
    rng = np.random.default_rng(3)
    with np.errstate(all="ignore"):
        dif = (rec[:, 0:3] * rng.random((W * H, 3)).astype(F)).astype(F)
        dh = (hv[:, :, 0:3] * rng.random((W * H, 2, 3)).astype(F)).astype(F)
    prm = DenoiseParams(iterations=3)
    got = atrous_denoise_split(rec, hv, dif, dh, al, W, H, prm)["records"]
    bad = ~np.isfinite(rec[:, 0:3]).all(-1)
    assert bad.sum() >= 6
    assert got[bad].tobytes() == rec[bad].tobytes()
    assert got[:, 3:].tobytes() == rec[:, 3:].tobytes()        # depth, normal and id are the record's bits
    # the finite pixels: the two filters, added once in binary32
    with np.errstate(all="ignore"):
        rest, direct = rec.copy(), rec.copy()
        rest[:, 0:3] = rec[:, 0:3] - dif
        direct[:, 0:3] = dif
        rh, dhh = hv.copy(), hv.copy()
        rh[:, :, 0:3] = hv[:, :, 0:3] - dh
        dhh[:, :, 0:3] = dh
        a = atrous_denoise(rest, rh, None, W, H, prm)["records"][:, 0:3]
        b = atrous_denoise(direct, dhh, al, W, H, prm)["records"][:, 0:3]
        want = (a + b).astype(F)
    assert got[~bad, 0:3].tobytes() == want[~bad].tobytes()
    assert not same_but_zero_sign(got, atrous_denoise(rec, hv, al, W, H, prm)["records"])     # (and it is neither of the plain filters)


def test_halves_and_diffuse_halves_come_together():
    W, H, rec, hv, al = FRAMES["random_clean"]
    n = W * H
    with pytest.raises(ValueError):
        atrous_denoise_split(rec, hv, np.zeros((n, 3), F), None, al, W, H)
    with pytest.raises(ValueError):
        atrous_denoise_split(rec, None, np.zeros((n, 3), F), np.zeros((n, 2, 3), F), al, W, H)


# ---- the ABI of the four new entry points
NAMES = ("rr_render_pixel_split", "rr_render_pixel_split_device", "rr_denoise_split_records", "rr_denoise_split_records_device")


def test_exported_bound_and_guarded():
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "rustray_hip.h")).read()
    src = host_api_source()
    for n in NAMES:
        assert n in capi.EXPORTS and hasattr(L, n) and getattr(L, n).argtypes is not None
        assert re.search(r"\bint " + n + r"\(rr_scene\* scene, ", header)
        assert re.search(r"\bint " + n + r"\([^{]*\) try \{", src), f"{n} is not a function-try-block"
        assert f'RR_GUARD_END("{n}")' in src
    assert "rr_api_pixel_split.h" in capi.LIB_SOURCES
    assert [len(getattr(L, n).argtypes) for n in NAMES] == [11, 12, 11, 12]
    assert "#define RR_ABI_VERSION 3u" in header


def test_python_layer_knows_the_diffuse_mode():
    from rustray_amd import renderer
    for ok in (False, True, "mean", "diffuse"):
        renderer._check_albedo_mode(ok)
    with pytest.raises(ValueError):
        renderer._check_albedo_mode("diffuse", temporal=True)
    with pytest.raises(ValueError):
        renderer._check_albedo_mode("centre")
    assert renderer._diffuse_mode("diffuse") and not renderer._diffuse_mode("mean") and not renderer._diffuse_mode(True)
